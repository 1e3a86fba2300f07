// Pipelined single frames (dr_pipeline_*, dr_render_accumulate_pipelined): groups of frames rendered on alternating streams, folded into the
// accumulator and presented in ticket order on a stream of their own.  Which ticket is where, what closes a group and what a launch waits for are
// pipeline_state.hpp's (the book of c->pipe): this file asks, turns the plans into stream waits and event records, and launches.
#include "context.hpp"

namespace dr {

int FramePipeline::setup(hipStream_t own) {
  if (ready) return DR_OK;
  // (a failed attempt leaves what it created in place -- the destructor releases it -- and `ready` false: the next call creates what is missing)
  bool ok = acc_stream || hipStreamCreateWithFlags(&acc_stream, hipStreamNonBlocking) == hipSuccess;
  stream[0] = own;
  for (int k = 1; k < PIPE_STREAMS; k++) ok = ok && (stream[k] || hipStreamCreateWithFlags(&stream[k], hipStreamNonBlocking) == hipSuccess);
  if (!ok) { set_error("pipeline: cannot create streams"); return DR_ERR_DEVICE; }
  auto event = [](hipEvent_t& e) { return e || hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess; };
  for (Slot& sl : slot) {
    ok = ok && event(sl.rendered);
    for (hipEvent_t& e : sl.added) ok = ok && event(e);
  }
  for (hipEvent_t& e : last) ok = ok && event(e);
  ok = ok && event(barrier) && event(sync);
  if (!ok) { set_error("pipeline: cannot create events"); return DR_ERR_DEVICE; }
  ready = true;
  return DR_OK;
}

void FramePipeline::drain() const {
  for (int k = 1; k < PIPE_STREAMS; k++) if (stream[k]) (void)hipStreamSynchronize(stream[k]);
  if (acc_stream) (void)hipStreamSynchronize(acc_stream);
}

FramePipeline::~FramePipeline() {
  for (Slot& sl : slot) {
    if (sl.rendered) (void)hipEventDestroy(sl.rendered);
    for (hipEvent_t e : sl.added) if (e) (void)hipEventDestroy(e);
  }
  for (hipEvent_t e : {last[0], last[1], last[2], last[3], barrier, sync}) if (e) (void)hipEventDestroy(e);
  for (int k = 1; k < PIPE_STREAMS; k++) if (stream[k]) (void)hipStreamDestroy(stream[k]);
  if (acc_stream) (void)hipStreamDestroy(acc_stream);
}

// how many frames a group may hold right now
int pipeline_group_room(const dr_context* c) {
  return group_room(c->pipe_group, !c->pipe_lean && uses_persistent(c) && persistent_can_store_per_frame(persistent_cfg(c, c->own_site())));
}

// Work queued through the pipeline runs on streams of its own: everything else (which uses `stream`) is ordered behind it here.
int join_pipeline(dr_context* c) {
  FramePipeline& p = c->pipe;
  if (!p.book.held.empty()) DR_TRY(pipeline_flush(c));
  const JoinPlan j = p.book.join_plan();
  for (int k = 0; k < j.n_adds; k++) HIP_TRY(hipStreamWaitEvent(c->stream, p.slot[j.slot[k]].added[j.frame[k]], 0));
  for (int q = 0; q < PIPE_STREAMS; q++) if (j.streams >> q & 1u) HIP_TRY(hipStreamWaitEvent(c->stream, p.last[q], 0));
  p.book.joined();
  return DR_OK;
}

}  // namespace dr

using namespace dr;

namespace {

// launches the first n held frames as one group
int pipeline_flush_some(dr_context* c, int n) {
  FramePipeline& p = c->pipe;
  const GroupBegin g = p.book.group_begin(n);
  FramePipeline::Slot& sl = p.slot[g.slot];
  const HeldFrame first = p.book.held[0];
  const int W = first.W, H = first.H;
  hipStream_t rs = p.stream[g.stream];
  LaunchSite site = {rs, false, c->pipe_lean != 0};      // (ODDITY: hold_order is decided below, after make_params, once the view's tiles are known)
  RenderParams P;
  DR_TRY(make_params(c, site, first.st, W, H, first.bg, first.seed, P, n));
  const size_t elems = (size_t)W * H * 3;
  const int tiles = P.ncols * P.gy;
  // the tile order and the costs it is made from are shared by all launches: a launch that refreshes them runs alone (after the other
  // streams' newest launches, and the launches after it wait for the refresh); all others read the order as it is.  The tile counters are
  // cleared (on this launch's stream) when the cursor wraps: like a refresh, that launch runs alone -- nobody may still count on the old values,
  // and nobody may start on the new ones before they are cleared
  const bool refresh = c->feedback && uses_persistent(c) && tiles > 0 && order_pipeline_refresh(c->order.state, view_key(c, P), tiles, c->feedback_every);
  site.hold_order = !refresh;
  const GroupPlan plan = p.book.group_plan(g, refresh, uses_persistent(c) && cursor_take(c->tile_cursor, c->queue_cursor_stride, c->queue_cursor_skew).wrap);
  // the waits for the slot: its previous group's adds must have run, and the presents nobody has waited for yet stay waitable (they park)
  if (plan.start_behind) {
    HIP_TRY(hipEventRecord(p.sync, c->stream));
    for (int q = 1; q < PIPE_STREAMS; q++) HIP_TRY(hipStreamWaitEvent(p.stream[q], p.sync, 0));
    HIP_TRY(hipStreamWaitEvent(p.acc_stream, p.sync, 0));
    p.book.started_behind();
  }
  if (plan.host_wait_slot) HIP_TRY(hipEventSynchronize(sl.added[plan.slot_last]));
  if (plan.stream_wait_slot) HIP_TRY(hipStreamWaitEvent(rs, sl.added[plan.slot_last], 0));
  p.book.group_take_slot(g, sl.rgb_host);
  // the buffers
  bool regrown;
  DR_TRY(sl.frames.fit(elems, n, n > c->pipe_group ? n : c->pipe_group, p.acc_stream, &regrown));      // (ODDITY: room for the option's group, whatever this one holds)
  if (regrown) sl.rect[0] = -1;
  // pixels outside the rendered block grid are 0 (K:2633-2636): the buffers are cleared when that grid changes, every frame of a grid
  // overwrites the same pixels (ODDITY: keyed by the rectangle alone, all cap_frames buffers at once)
  const int rect[6] = {W, H, P.gx, P.gy, P.stripe_mod, P.stripe_rem};
  if (memcmp(rect, sl.rect, sizeof(rect)) != 0) {
    HIP_TRY(hipMemsetAsync(sl.frames, 0, (size_t)sl.frames.cap_frames * elems * sizeof(int32_t), rs));
    memcpy(sl.rect, rect, sizeof(rect));
  }
  P.out = sl.frames;
  P.accumulate = 0;
  P.batch = n; P.batch_seed_stride = g.seed_stride;
  P.out_frame_stride = n > 1 ? (uint32_t)elems : 0u;      // (ODDITY: a group of one is an ordinary launch: every build can render it)
  // the waits for the launch, the launch, its records
  if (plan.wait_barrier) HIP_TRY(hipStreamWaitEvent(rs, p.barrier, 0));
  for (int q = 0; q < PIPE_STREAMS; q++) if (plan.wait_streams >> q & 1u) HIP_TRY(hipStreamWaitEvent(rs, p.last[q], 0));
  if (tiles > 0) {
    DR_TRY(enqueue_frame(c, site, P));
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipEventRecord(p.last[g.stream], rs));
  if (plan.alone) HIP_TRY(hipEventRecord(p.barrier, rs));
  HIP_TRY(hipEventRecord(sl.rendered, rs));
  // fold into the accumulator, in ticket order (K:2213-2218), and make the image of exactly the frames so far (K:2287)
  HIP_TRY(hipStreamWaitEvent(p.acc_stream, sl.rendered, 0));
  for (int f = 0; f < n; f++) {
    if (c->m2) launch_moments_add(p.acc_stream, c->accum, sl.frames + (size_t)f * elems, c->m2, (size_t)W * H);      // acc += frame; M2 += yc^2
    else launch_frame_add(p.acc_stream, c->accum, sl.frames + (size_t)f * elems, elems);
    if (const int div = p.book.held[(size_t)f].div) {
      const size_t bytes = (size_t)W * H * 3;
      DR_TRY(sl.rgb_dev[f].grow(bytes, p.acc_stream));
      DR_TRY(sl.rgb_host[f].grow(bytes, p.acc_stream));
      launch_present(p.acc_stream, c->accum, c->hist, sl.rgb_dev[f], W, H, div);
      HIP_TRY(hipMemcpyAsync(sl.rgb_host[f], sl.rgb_dev[f], bytes, hipMemcpyDeviceToHost, p.acc_stream));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sl.added[f], p.acc_stream));
  }
  p.book.group_commit(g, plan);
  c->stats.launches += tiles > 0 ? 1 : 0;
  c->stats.frames += (uint64_t)n;
  c->stats.samples += (uint64_t)(tiles > 0 ? tiles : 0) * 64ull * (uint64_t)(P.spp_f > 0 ? ceilf(P.spp_f) : 0) * (uint64_t)n;
  return DR_OK;
}

}  // namespace

namespace dr {

// launches the frames submitted since the last launch.  Whatever changes the state a launch reads -- the scene, the stripe, the traversal, the
// counters switch, an option -- calls this before it changes it, so the frames run with the state they were submitted under, as ONE group
// (TicketBook::flush_size).  A launch that fails drops what is still held
int pipeline_flush(dr_context* c) {
  TicketBook<FramePipeline::Image>& book = c->pipe.book;
  while (!book.held.empty()) {
    const int rc = pipeline_flush_some(c, book.flush_size(pipeline_group_room(c)));
    if (rc != DR_OK) { book.drop_held(); return rc; }
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
  DR_TRY(c->pipe.setup(c->stream));
  if (c->traversal == DR_TRAVERSAL_ORDERED && c->tree_depth > ORDERED_STACK) { set_error("tree too deep for ordered traversal"); return DR_ERR_SCENE; }
  {   // a frame that cannot be rendered must fail here, not when its group is launched
    RenderParams probe;
    DR_TRY(make_params(c, c->own_site(), settings13, W, H, background, frame_seed, probe, 1));
  }
  TicketBook<FramePipeline::Image>& book = c->pipe.book;
  const bool closes = book.submit_closes(settings13, W, H, background, frame_seed);
  // every ticket handed out stays waitable: a frame whose launches could overfill the store of parked images is refused, never an image dropped
  if (book.submit_overfills(closes)) {
    set_error("pipeline: too many presented frames have not been waited for: call dr_pipeline_wait for the oldest tickets first");
    return DR_ERR_INVALID;
  }
  if (closes) DR_TRY(pipeline_flush(c));
  const uint64_t k = book.hold(settings13, W, H, background, frame_seed, present_divide_by);
  if (ticket) *ticket = k;
  if (book.group_full(pipeline_group_room(c))) return pipeline_flush(c);
  return DR_OK;
}

int dr_pipeline_wait(dr_context* c, uint64_t ticket, uint8_t* out_rgb8) {
  if (!c || !c->pipe.ready) { set_error("pipeline: nothing submitted"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  FramePipeline& p = c->pipe;
  TicketAt at = p.book.locate(ticket);
  if (at.place == TICKET_HELD) { DR_TRY(pipeline_flush(c)); at = p.book.locate(ticket); }      // submitted, its group not launched yet: it is now
  const size_t bytes = (size_t)c->accW * c->accH * 3;
  switch (at.place) {
    case TICKET_SLOT: {
      FramePipeline::Slot& sl = p.slot[at.slot];
      HIP_TRY(hipEventSynchronize(sl.added[at.frame]));
      const bool presented = p.book.mark_waited(at, ticket);
      if (out_rgb8) {
        if (!presented) { set_error("pipeline: that frame was submitted without a present"); return DR_ERR_INVALID; }
        memcpy(out_rgb8, sl.rgb_host[at.frame], bytes);
      }
      return DR_OK;
    }
    case TICKET_PARKED: {      // its slot has been reused: the frame has been added (the launch that took the slot waited for that), and its image was kept
      p.book.mark_waited(at, ticket);
      const FramePipeline::Image& rgb = *p.book.parked_image(at, ticket);
      if (out_rgb8) memcpy(out_rgb8, rgb, bytes < rgb.n ? bytes : rgb.n);
      return DR_OK;
    }
    case TICKET_FINISHED:
      if (out_rgb8) { set_error("pipeline: that frame was submitted without a present (or its image was handed out by an earlier wait and has been released)"); return DR_ERR_INVALID; }
      return DR_OK;
    default:
      set_error("pipeline: no such ticket (dr_pipeline_submit has not handed it out)");
      return DR_ERR_INVALID;
  }
}

int dr_pipeline_image(dr_context* c, uint64_t ticket, const uint8_t** rgb8) {
  if (!c || !c->pipe.ready || !rgb8) { set_error("pipeline: nothing submitted, or null argument"); return DR_ERR_INVALID; }
  const FramePipeline& p = c->pipe;
  const TicketAt at = p.book.locate(ticket);
  if (at.place != TICKET_SLOT && at.place != TICKET_PARKED) {
    set_error("pipeline: no image of that ticket (not handed out, submitted without a present, or released after its wait)");
    return DR_ERR_INVALID;
  }
  if (!p.book.waited(at, ticket)) { set_error("pipeline: dr_pipeline_wait(ticket) comes first"); return DR_ERR_INVALID; }
  if (!p.book.presented(at)) { set_error("pipeline: that frame was submitted without a present"); return DR_ERR_INVALID; }
  const FramePipeline::Image* parked = p.book.parked_image(at, ticket);
  *rgb8 = parked ? *parked : p.slot[at.slot].rgb_host[at.frame];
  return DR_OK;
}

int dr_render_accumulate_pipelined(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed,
                                   uint64_t seed_stride, int nframes) {
  if (!c || nframes < 0) { set_error("bad argument"); return DR_ERR_INVALID; }
  uint64_t last = 0;
  for (int k = 0; k < nframes; k++) DR_TRY(dr_pipeline_submit(c, settings13, W, H, background, frame_seed + (uint64_t)k * seed_stride, 0, &last));
  if (nframes > 0) {
    DR_TRY(dr_pipeline_wait(c, last, nullptr));      // adds run in order: the last one ends the batch
    c->pipe.book.all_drained();
  }
  return DR_OK;
}

}  // extern "C"
