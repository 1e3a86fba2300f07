// pipeline_state.hpp on the host (tests/test_pipeline_state_host.py, tools/host_sanitize_driver.cpp): the ticket book behind a handle, a frame's image
// an integer token -- so a test can tell whose image a wait hands back --, the slots' images (the context's pinned buffers) beside it, and the group
// between group_begin and group_commit.  A view is an integer: settings13[0] = view % 4, background = view / 4 % 2, W = 96 + 8 * (view / 8 % 2), H = 64.
// Part of host_kernel.cpp.
struct HkPipeline {
  TicketBook<long long> book;
  long long image[PIPE_DEPTH][PIPE_GROUP_MAX] = {{0}};
  GroupBegin g;
  GroupPlan plan;
};
struct HkView { float st[13]; int W, H; float bg; };
static HkView hk_pipeline_view(int view) {
  HkView v = {{0}, 96 + 8 * (view / 8 % 2), 64, (float)(view / 4 % 2)};
  v.st[0] = (float)(view % 4);
  return v;
}
extern "C" {
void* hk_pipeline_new() { return new HkPipeline(); }
void hk_pipeline_free(void* h) { delete (HkPipeline*)h; }
int hk_pipeline_parked_max() { return PIPE_PARKED_MAX; }
int hk_pipeline_group_room(int pipe_group, int can_store_per_frame) { return group_room(pipe_group, can_store_per_frame != 0); }
// locate: out5 = place (TicketPlace), slot, frame, dr_pipeline_wait has returned for it (slot and parked), it was presented (slot; parked: 1)
void hk_pipeline_locate(void* h, uint64_t ticket, int* out5) {
  const TicketBook<long long>& b = ((HkPipeline*)h)->book;
  const TicketAt at = b.locate(ticket);
  const bool has = at.place == TICKET_SLOT || at.place == TICKET_PARKED;
  out5[0] = at.place; out5[1] = at.slot; out5[2] = at.frame; out5[3] = has && b.waited(at, ticket); out5[4] = has && b.presented(at);
}
int hk_pipeline_submit_closes(void* h, int view, uint64_t seed) {
  const HkView v = hk_pipeline_view(view);
  return ((HkPipeline*)h)->book.submit_closes(v.st, v.W, v.H, v.bg, seed) ? 1 : 0;
}
int hk_pipeline_owed_after(void* h, int launches) { return ((HkPipeline*)h)->book.owed_after(launches); }
int hk_pipeline_submit_overfills(void* h, int closes) { return ((HkPipeline*)h)->book.submit_overfills(closes != 0) ? 1 : 0; }
uint64_t hk_pipeline_hold(void* h, int view, uint64_t seed, int div) {
  const HkView v = hk_pipeline_view(view);
  return ((HkPipeline*)h)->book.hold(v.st, v.W, v.H, v.bg, seed, div);
}
int hk_pipeline_group_full(void* h, int room) { return ((HkPipeline*)h)->book.group_full(room) ? 1 : 0; }
int hk_pipeline_flush_size(void* h, int room) { return ((HkPipeline*)h)->book.flush_size(room); }
void hk_pipeline_drop_held(void* h) { ((HkPipeline*)h)->book.drop_held(); }
// group_begin: out = slot, stream, first ticket, seed stride, frames to park, then those frames
void hk_pipeline_group_begin(void* h, int n, long long* out) {
  HkPipeline& p = *(HkPipeline*)h;
  p.g = p.book.group_begin(n);
  out[0] = p.g.slot; out[1] = p.g.stream; out[2] = (long long)p.g.first_ticket; out[3] = (long long)p.g.seed_stride; out[4] = p.g.n_park;
  for (int k = 0; k < p.g.n_park; k++) out[5 + k] = p.g.park[k];
}
// group_plan of the group begun: out7 = start_behind, host_wait_slot, stream_wait_slot, slot_last, wait_barrier, alone, wait_streams
void hk_pipeline_group_plan(void* h, int refresh, int cursor_wraps, int* out7) {
  HkPipeline& p = *(HkPipeline*)h;
  p.plan = p.book.group_plan(p.g, refresh != 0, cursor_wraps != 0);
  const int v[7] = {p.plan.start_behind, p.plan.host_wait_slot, p.plan.stream_wait_slot, p.plan.slot_last, p.plan.wait_barrier, p.plan.alone, (int)p.plan.wait_streams};
  memcpy(out7, v, sizeof(v));
}
// what follows the plan's first waits: started_behind if the plan says so, then group_take_slot
void hk_pipeline_group_take_slot(void* h) {
  HkPipeline& p = *(HkPipeline*)h;
  if (p.plan.start_behind) p.book.started_behind();
  p.book.group_take_slot(p.g, p.image[p.g.slot]);
}
// the presents (the token of frame f becomes the slot's image f, for the frames held with a divisor) and group_commit
void hk_pipeline_group_commit(void* h, const long long* tokens) {
  HkPipeline& p = *(HkPipeline*)h;
  for (int f = 0; f < p.g.n; f++) if (p.book.held[(size_t)f].div != 0) p.image[p.g.slot][f] = tokens[f];
  p.book.group_commit(p.g, p.plan);
}
// mark_waited of a ticket in a slot or parked: 1 when the frame has an image
int hk_pipeline_mark_waited(void* h, uint64_t ticket) {
  TicketBook<long long>& b = ((HkPipeline*)h)->book;
  return b.mark_waited(b.locate(ticket), ticket) ? 1 : 0;
}
// the image dr_pipeline_wait / dr_pipeline_image hand out for a ticket in a slot or parked
long long hk_pipeline_image(void* h, uint64_t ticket) {
  const HkPipeline& p = *(HkPipeline*)h;
  const TicketAt at = p.book.locate(ticket);
  const long long* parked = p.book.parked_image(at, ticket);
  return parked ? *parked : p.image[at.slot][at.frame];
}
void hk_pipeline_all_drained(void* h) { ((HkPipeline*)h)->book.all_drained(); }
// join_plan, then joined: out = the adds waited for, (slot, frame) of each, and last the streams' mask -- 2 + 2 * adds words
void hk_pipeline_join(void* h, int* out) {
  TicketBook<long long>& b = ((HkPipeline*)h)->book;
  const JoinPlan j = b.join_plan();
  *out++ = j.n_adds;
  for (int k = 0; k < j.n_adds; k++) { *out++ = j.slot[k]; *out++ = j.frame[k]; }
  *out = (int)j.streams;
  b.joined();
}
void hk_pipeline_restart_numbering(void* h, int streams) { ((HkPipeline*)h)->book.restart_numbering(streams); }
// the whole book, at most `room` words of it; returns the words there are: next, groups, streams, dirty, barrier_set, last_set[4]; held frames n, then
// per frame settings13[0], W, H, background, seed, div; per slot first, count, unwaited, drained, div[16], fwaited[16], image[16]; parked n, then per
// entry ticket, waited, image
int hk_pipeline_dump(void* h, long long* out, int room) {
  const HkPipeline& p = *(HkPipeline*)h;
  const TicketBook<long long>& b = p.book;
  std::vector<long long> w = {(long long)b.next, (long long)b.groups, b.streams, b.dirty, b.barrier_set};
  for (bool s : b.last_set) w.push_back(s);
  w.push_back((long long)b.held.size());
  for (const HeldFrame& f : b.held) w.insert(w.end(), {(long long)f.st[0], f.W, f.H, (long long)f.bg, (long long)f.seed, f.div});
  for (int k = 0; k < PIPE_DEPTH; k++) {
    const SlotBook& s = b.slot[k];
    w.insert(w.end(), {(long long)s.first, s.count, s.unwaited, s.drained});
    for (int d : s.div) w.push_back(d);
    for (bool f : s.fwaited) w.push_back(f);
    for (long long i : p.image[k]) w.push_back(i);
  }
  w.push_back((long long)b.parked.size());
  for (const auto& kv : b.parked) w.insert(w.end(), {(long long)kv.first, kv.second.waited, kv.second.image});
  if (out) memcpy(out, w.data(), sizeof(long long) * (size_t)((int)w.size() < room ? (int)w.size() : room));
  return (int)w.size();
}
}  // extern "C"
