// Pipelined single frames (dr_pipeline_*, dr_render_accumulate_pipelined): groups of frames rendered on alternating streams, folded into the
// accumulator and presented in ticket order on a stream of their own.
#include "context.hpp"

namespace dr {

// Work queued through the pipeline runs on two more streams: everything else (which uses `stream`) is ordered behind it here.
int join_pipeline(dr_context* c) {
  if (!c->pipe_pending.empty()) DR_TRY(pipeline_flush(c));
  if (!c->pipe_dirty) return DR_OK;
  for (int k = 0; k < dr_context::PIPE_DEPTH; k++) {
    const dr_context::PipeSlot& sl = c->pipe_slot[k];
    if (sl.count > 0) HIP_TRY(hipStreamWaitEvent(c->stream, sl.added[sl.count - 1], 0));      // (adds run in order: the last one ends the group)
  }
  for (int k = 1; k < dr_context::PIPE_STREAMS; k++) if (c->pipe_last_set[k]) HIP_TRY(hipStreamWaitEvent(c->stream, c->pipe_last[k], 0));
  c->pipe_dirty = false;
  return DR_OK;
}

}  // namespace dr

using namespace dr;

namespace {

int pipeline_setup(dr_context* c) {
  if (c->pipe_ready) return DR_OK;
  // (a failed attempt leaves what it created in place -- dr_context_destroy releases it -- and pipe_ready false: the next call creates what is missing)
  bool ok = c->acc_stream || hipStreamCreateWithFlags(&c->acc_stream, hipStreamNonBlocking) == hipSuccess;
  c->pipe_stream[0] = c->stream;
  for (int k = 1; k < dr_context::PIPE_STREAMS; k++) ok = ok && (c->pipe_stream[k] || hipStreamCreateWithFlags(&c->pipe_stream[k], hipStreamNonBlocking) == hipSuccess);
  if (!ok) { set_error("pipeline: cannot create streams"); return DR_ERR_DEVICE; }
  auto event = [](hipEvent_t& e) { return e || hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess; };
  for (int k = 0; k < dr_context::PIPE_DEPTH; k++) {
    ok = ok && event(c->pipe_slot[k].rendered);
    for (int f = 0; f < dr_context::PIPE_GROUP_MAX; f++) ok = ok && event(c->pipe_slot[k].added[f]);
  }
  for (int k = 0; k < dr_context::PIPE_STREAMS; k++) ok = ok && event(c->pipe_last[k]);
  ok = ok && event(c->pipe_barrier) && event(c->pipe_sync);
  if (!ok) { set_error("pipeline: cannot create events"); return DR_ERR_DEVICE; }
  c->pipe_ready = true;
  return DR_OK;
}

// how many frames a group may hold right now: the option, if the launch configuration has the builds that store every frame of a batch separately
int pipeline_group_size(const dr_context* c) {
  if (c->pipe_group <= 1 || c->pipe_lean || !uses_persistent(c) || !persistent_can_store_per_frame(persistent_cfg(c, c->own_site()))) return 1;
  return c->pipe_group;
}

// the slot that holds a launched ticket (null: not in flight any more, or still pending)
dr_context::PipeSlot* pipeline_slot_of(dr_context* c, uint64_t ticket) {
  for (dr_context::PipeSlot& sl : c->pipe_slot)
    if (sl.count > 0 && ticket >= sl.first && ticket < sl.first + (uint64_t)sl.count) return &sl;
  return nullptr;
}

// A slot is about to be reused and the host has waited for its last add: the images of its frames that were presented and have not been waited for
// are still owed to the caller.  They move to the context's store (the pinned buffers are swapped, not copied); the slot, which then holds no ticket,
// allocates new ones.
void pipeline_park(dr_context* c, dr_context::PipeSlot& sl) {
  for (int f = 0; f < sl.count; f++)
    if (sl.div[f] != 0 && !sl.fwaited[f]) {
      dr_context::PipeParked& e = c->pipe_parked[sl.first + (uint64_t)f];
      e.rgb.swap(sl.rgb_host[f]);
      e.waited = false;
    }
  sl.unwaited = 0; sl.count = 0;
}

// images owed to the caller that would be in the store after the next `launches` launches: those in it now and not waited for, and those of the slots
// these launches reuse
int pipeline_owed_after(const dr_context* c, int launches) {
  int owed = 0;
  for (const auto& kv : c->pipe_parked) owed += kv.second.waited ? 0 : 1;
  const uint64_t depth = (uint64_t)c->pipe_streams + 1;
  for (int k = 0; k < launches && k < (int)depth; k++) owed += c->pipe_slot[(c->pipe_groups + (uint64_t)k) % depth].unwaited;
  return owed;
}

// launches the first n pending frames as one group
int pipeline_flush_some(dr_context* c, int n) {
  if (!c->pipe_parked.empty())                // images that have been waited for were the caller's until now
    for (auto it = c->pipe_parked.begin(); it != c->pipe_parked.end();) it = it->second.waited ? c->pipe_parked.erase(it) : std::next(it);
  const dr_context::PipePending first = c->pipe_pending[0];
  const uint64_t stride = n > 1 ? c->pipe_pending[1].seed - first.seed : 0;
  const uint64_t first_ticket = c->pipe_next - (uint64_t)c->pipe_pending.size();
  const int W = first.W, H = first.H;
  const uint64_t g = c->pipe_groups;
  const int nstreams = c->pipe_streams, depth = nstreams + 1;
  const int si = (int)(g % (uint64_t)nstreams);
  dr_context::PipeSlot& sl = c->pipe_slot[g % (uint64_t)depth];
  hipStream_t rs = c->pipe_stream[si];
  LaunchSite site = {rs, false, c->pipe_lean != 0};      // (hold_order: decided below, once the view's tiles are known)
  RenderParams P;
  DR_TRY(make_params(c, site, first.st, W, H, first.bg, first.seed, P, n));
  const size_t elems = (size_t)W * H * 3;
  if (!c->pipe_dirty) {                       // the first group after other work: the pipeline's streams start behind it
    HIP_TRY(hipEventRecord(c->pipe_sync, c->stream));
    for (int q = 1; q < dr_context::PIPE_STREAMS; q++) HIP_TRY(hipStreamWaitEvent(c->pipe_stream[q], c->pipe_sync, 0));
    HIP_TRY(hipStreamWaitEvent(c->acc_stream, c->pipe_sync, 0));
    c->pipe_dirty = true;
  }
  // the slot's previous group: its adds must have run, and the presents nobody has waited for yet stay waitable
  if (!sl.drained && sl.count > 0) { HIP_TRY(hipEventSynchronize(sl.added[sl.count - 1])); sl.drained = true; }
  if (sl.count > 0) HIP_TRY(hipStreamWaitEvent(rs, sl.added[sl.count - 1], 0));
  if (sl.unwaited > 0) pipeline_park(c, sl);
  if (sl.elems_each != elems || sl.cap_frames < n || !sl.frames) {
    const int cap = n > c->pipe_group ? n : c->pipe_group;
    sl.cap_frames = 0;
    DR_TRY(sl.frames.grow((size_t)cap * elems, c->acc_stream));
    sl.elems_each = elems; sl.cap_frames = cap;
    sl.rect[0] = -1;
  }
  // pixels outside the rendered block grid are 0 (K:2633-2636): the buffers are cleared when that grid changes, every frame of a grid
  // overwrites the same pixels
  const int rect[6] = {W, H, P.gx, P.gy, P.stripe_mod, P.stripe_rem};
  if (memcmp(rect, sl.rect, sizeof(rect)) != 0) {
    HIP_TRY(hipMemsetAsync(sl.frames, 0, (size_t)sl.cap_frames * elems * sizeof(int32_t), rs));
    memcpy(sl.rect, rect, sizeof(rect));
  }
  P.out = sl.frames;
  P.accumulate = 0;
  P.batch = n; P.batch_seed_stride = stride;
  P.out_frame_stride = n > 1 ? (uint32_t)elems : 0u;      // (a group of one is an ordinary launch: every build can render it)
  const int tiles = P.ncols * P.gy;
  // the tile order and the costs it is made from are shared by all launches: a launch that refreshes them runs alone (after the other
  // streams' newest launches, and the launches after it wait for the refresh); all others read the order as it is
  const bool refresh = c->feedback && uses_persistent(c) && tiles > 0 && order_pipeline_refresh(c->order.state, view_key(c, P), tiles, c->feedback_every);
  site.hold_order = !refresh;
  if (c->pipe_barrier_set) HIP_TRY(hipStreamWaitEvent(rs, c->pipe_barrier, 0));
  // the tile counters are cleared (on this launch's stream) when the cursor wraps: like a refresh, that launch runs alone -- nobody may
  // still count on the old values, and nobody may start on the new ones before they are cleared
  const bool alone = refresh || c->tile_cursor + LAUNCH_COUNTERS > TILE_COUNTERS;
  if (alone)
    for (int q = 0; q < dr_context::PIPE_STREAMS; q++) if (q != si && c->pipe_last_set[q]) HIP_TRY(hipStreamWaitEvent(rs, c->pipe_last[q], 0));
  if (tiles > 0) {
    DR_TRY(enqueue_frame(c, site, P));
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(c->pipe_last[si], rs)); c->pipe_last_set[si] = true;
  if (alone) { HIP_TRY(hipEventRecord(c->pipe_barrier, rs)); c->pipe_barrier_set = true; }
  HIP_TRY(hipEventRecord(sl.rendered, rs));
  // fold into the accumulator, in ticket order (K:2213-2218), and make the image of exactly the frames so far (K:2287)
  HIP_TRY(hipStreamWaitEvent(c->acc_stream, sl.rendered, 0));
  sl.unwaited = 0;
  for (int f = 0; f < n; f++) {
    if (c->m2) launch_moments_add(c->acc_stream, c->accum, sl.frames + (size_t)f * elems, c->m2, (size_t)W * H);      // acc += frame; M2 += yc^2
    else launch_frame_add(c->acc_stream, c->accum, sl.frames + (size_t)f * elems, elems);
    const int div = c->pipe_pending[(size_t)f].div;
    sl.div[f] = 0; sl.fwaited[f] = false;
    if (div != 0) {
      const size_t bytes = (size_t)W * H * 3;
      DR_TRY(sl.rgb_dev[f].grow(bytes, c->acc_stream));
      DR_TRY(sl.rgb_host[f].grow(bytes, c->acc_stream));
      launch_present(c->acc_stream, c->accum, c->hist, sl.rgb_dev[f], W, H, div);
      HIP_TRY(hipMemcpyAsync(sl.rgb_host[f], sl.rgb_dev[f], bytes, hipMemcpyDeviceToHost, c->acc_stream));
      sl.div[f] = div;
      sl.unwaited++;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sl.added[f], c->acc_stream));
  }
  sl.first = first_ticket; sl.count = n; sl.drained = false;
  c->pipe_groups = g + 1;
  c->stats.launches += tiles > 0 ? 1 : 0;
  c->stats.frames += (uint64_t)n;
  c->stats.samples += (uint64_t)(tiles > 0 ? tiles : 0) * 64ull * (uint64_t)(P.spp_f > 0 ? ceilf(P.spp_f) : 0) * (uint64_t)n;
  c->pipe_pending.erase(c->pipe_pending.begin(), c->pipe_pending.begin() + n);
  return DR_OK;
}

}  // namespace

namespace dr {

// launches the frames submitted since the last launch, as ONE group.  Whatever changes the state a launch reads -- the scene, the stripe, the traversal,
// the counters switch, an option -- calls this before it changes it, so the frames run with the state they were submitted under and the configuration
// still has the builds that store every frame of a batch separately.  Were it not so, they would be launched one by one (a defence: no caller gets there)
int pipeline_flush(dr_context* c) {
  while (!c->pipe_pending.empty()) {
    const int all = (int)c->pipe_pending.size();
    const int rc = pipeline_flush_some(c, pipeline_group_size(c) >= all ? all : 1);
    if (rc != DR_OK) { c->pipe_pending.clear(); return rc; }
  }
  return DR_OK;
}

}  // namespace dr

extern "C" {

int dr_pipeline_submit(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed, int present_divide_by,
                       uint64_t* ticket) {
  if (!c || !settings13) { set_error("null argument"); return DR_ERR_INVALID; }
  if (!c->accum || c->accW != W || c->accH != H) { set_error("call dr_accum_reset(W, H) first"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(pipeline_setup(c));
  if (c->traversal == DR_TRAVERSAL_ORDERED && c->tree_depth > ORDERED_STACK) { set_error("tree too deep for ordered traversal"); return DR_ERR_SCENE; }
  {   // a frame that cannot be rendered must fail here, not when its group is launched
    RenderParams probe;
    DR_TRY(make_params(c, c->own_site(), settings13, W, H, background, frame_seed, probe, 1));
  }
  // a group holds frames of ONE view whose seeds are in arithmetic progression (what a progressive render submits): anything else starts a new group
  bool closes = false;
  if (!c->pipe_pending.empty()) {
    const dr_context::PipePending& p0 = c->pipe_pending[0];
    const dr_context::PipePending& pl = c->pipe_pending.back();
    const bool same_view = memcmp(p0.st, settings13, 13 * sizeof(float)) == 0 && p0.W == W && p0.H == H && p0.bg == background;
    const bool in_step = c->pipe_pending.size() == 1 || frame_seed - pl.seed == c->pipe_pending[1].seed - p0.seed;
    closes = !same_view || !in_step;
  }
  // every ticket handed out stays waitable: the launch of the group this frame closes and the launch of its own group each reuse a slot, and the
  // presents of those slots that nobody has waited for go to the store.  A frame that could overfill it is refused, never an image dropped
  if (pipeline_owed_after(c, closes ? 2 : 1) > dr_context::PIPE_PARKED_MAX) {
    set_error("pipeline: too many presented frames have not been waited for: call dr_pipeline_wait for the oldest tickets first");
    return DR_ERR_INVALID;
  }
  if (closes) DR_TRY(pipeline_flush(c));
  dr_context::PipePending p;
  memcpy(p.st, settings13, sizeof(p.st)); p.W = W; p.H = H; p.bg = background; p.seed = frame_seed; p.div = present_divide_by;
  c->pipe_pending.push_back(p);
  const uint64_t k = c->pipe_next;
  c->pipe_next = k + 1;
  if (ticket) *ticket = k;
  if ((int)c->pipe_pending.size() >= pipeline_group_size(c)) return pipeline_flush(c);
  return DR_OK;
}

int dr_pipeline_wait(dr_context* c, uint64_t ticket, uint8_t* out_rgb8) {
  if (!c || !c->pipe_ready) { set_error("pipeline: nothing submitted"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  if (ticket < c->pipe_next && ticket + c->pipe_pending.size() >= c->pipe_next) DR_TRY(pipeline_flush(c));      // submitted, its group not launched yet: it is now
  const size_t bytes = (size_t)c->accW * c->accH * 3;
  if (dr_context::PipeSlot* sl = pipeline_slot_of(c, ticket)) {
    const int f = (int)(ticket - sl->first);
    HIP_TRY(hipEventSynchronize(sl->added[f]));
    if (!sl->fwaited[f] && sl->div[f]) sl->unwaited--;
    sl->fwaited[f] = true;
    if (f == sl->count - 1) sl->drained = true;
    if (out_rgb8) {
      if (!sl->div[f]) { set_error("pipeline: that frame was submitted without a present"); return DR_ERR_INVALID; }
      memcpy(out_rgb8, sl->rgb_host[f], bytes);
    }
    return DR_OK;
  }
  // its slot has been reused: the frame has been added (the launch that took the slot waited for that), and its image, if it is still owed, was kept
  auto parked = c->pipe_parked.find(ticket);
  if (parked != c->pipe_parked.end()) {
    parked->second.waited = true;
    if (out_rgb8) memcpy(out_rgb8, parked->second.rgb, bytes < parked->second.rgb.n ? bytes : parked->second.rgb.n);
    return DR_OK;
  }
  if (ticket >= c->pipe_next - c->pipe_pending.size()) { set_error("pipeline: no such ticket (dr_pipeline_submit has not handed it out)"); return DR_ERR_INVALID; }
  if (out_rgb8) { set_error("pipeline: that frame was submitted without a present (or its image was handed out by an earlier wait and has been released)"); return DR_ERR_INVALID; }
  return DR_OK;
}

int dr_pipeline_image(dr_context* c, uint64_t ticket, const uint8_t** rgb8) {
  if (!c || !c->pipe_ready || !rgb8) { set_error("pipeline: nothing submitted, or null argument"); return DR_ERR_INVALID; }
  dr_context::PipeSlot* sl = pipeline_slot_of(c, ticket);
  if (!sl) {
    auto parked = c->pipe_parked.find(ticket);
    if (parked == c->pipe_parked.end()) { set_error("pipeline: no image of that ticket (not handed out, submitted without a present, or released after its wait)"); return DR_ERR_INVALID; }
    if (!parked->second.waited) { set_error("pipeline: dr_pipeline_wait(ticket) comes first"); return DR_ERR_INVALID; }
    *rgb8 = parked->second.rgb;
    return DR_OK;
  }
  const int f = (int)(ticket - sl->first);
  if (!sl->fwaited[f]) { set_error("pipeline: dr_pipeline_wait(ticket) comes first"); return DR_ERR_INVALID; }
  if (!sl->div[f]) { set_error("pipeline: that frame was submitted without a present"); return DR_ERR_INVALID; }
  *rgb8 = sl->rgb_host[f];
  return DR_OK;
}

int dr_render_accumulate_pipelined(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed,
                                   uint64_t seed_stride, int nframes) {
  if (!c || nframes < 0) { set_error("bad argument"); return DR_ERR_INVALID; }
  uint64_t last = 0;
  for (int k = 0; k < nframes; k++) DR_TRY(dr_pipeline_submit(c, settings13, W, H, background, frame_seed + (uint64_t)k * seed_stride, 0, &last));
  if (nframes > 0) {
    DR_TRY(dr_pipeline_wait(c, last, nullptr));      // adds run in order: the last one ends the batch
    for (dr_context::PipeSlot& sl : c->pipe_slot) sl.drained = true;
  }
  return DR_OK;
}

}  // extern "C"
