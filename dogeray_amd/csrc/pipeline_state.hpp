// The pipelined present loop's bookkeeping (dr_pipeline_*) as plain data: the ticket book -- which frame is held, in which slot, parked,
// finished --, the rules that close and size a group, and the ordering plan of a group's launch and of a join.  No HIP: dr_context's FramePipeline
// (context.hpp) holds streams, events and buffers, context_pipeline.cpp turns a plan into hipStreamWaitEvent / hipEventRecord calls, and the host
// build exports the book with an integer for the image (tests/test_pipeline_state_host.py).  ODDITY marks behaviour nobody would write on purpose
// that is kept, as in launch_state.hpp.
#pragma once
#include <cstdint>
#include <cstring>
#include <iterator>
#include <map>
#include <utility>
#include <vector>

namespace dr {

constexpr int PIPE_STREAMS = 4;                      // render streams at most (the context's own is number 0); option pipe_streams uses 2 .. 4 of them
constexpr int PIPE_DEPTH = PIPE_STREAMS + 1;         // slots: a numbering under s streams rotates through s + 1 of them
constexpr int PIPE_GROUP_MAX = 16;                   // frames per group at most (option pipe_group)
constexpr int PIPE_PARKED_MAX = 2 * PIPE_GROUP_MAX;  // images owed to the caller whose slot has been reused: a submit that could leave more is refused

// a frame submitted and not launched yet
struct HeldFrame { float st[13]; int W, H; float bg; uint64_t seed; int div; };

// a slot = one GROUP of frames in flight: frames submitted one after the other (same view, seeds in arithmetic progression) share one launch and are
// added to the accumulator and presented one by one, in ticket order
struct SlotBook {
  uint64_t first = 0; int count = 0;               // tickets [first, first + count)
  int div[PIPE_GROUP_MAX] = {0};                   // divisor frame f was presented with (0: not presented)
  bool fwaited[PIPE_GROUP_MAX] = {false};          // dr_pipeline_wait has returned for frame f
  int unwaited = 0;                                // frames of the group that were presented and have not been waited for: their images are owed
  bool drained = true;                             // the host has waited for the group's last add: its buffers may be reused at once
};

// where a ticket is
enum TicketPlace {
  TICKET_HELD,               // submitted, its group not launched yet
  TICKET_SLOT,               // frame `frame` of the group in slot `slot`
  TICKET_PARKED,             // its slot has been reused; its image, still owed, is in the store
  TICKET_FINISHED,           // handed out, added, and no image owed: never presented, or released after its wait (or dropped by a failed flush)
  TICKET_NEVER               // dr_pipeline_submit has not handed it out
};
struct TicketAt { TicketPlace place; int slot, frame; };

// the group the next launch renders, and where
struct GroupBegin {
  int n;                     // frames: the first n held ones
  int slot, stream;          // group % (streams + 1), group % streams
  uint64_t first_ticket, seed_stride;
  int n_park, park[PIPE_GROUP_MAX];      // frames of the slot's previous group whose images will be parked (presented, not waited for)
};

// What a group's launch on `stream` waits for and records, in the order context_pipeline.cpp issues it
struct GroupPlan {
  bool start_behind;         // the first group after other work: every pipeline stream waits for what `stream` holds now
  bool host_wait_slot;       // the host waits for the last add of the slot's previous group (its buffers are reused) ...
  bool stream_wait_slot;     // ... and so does the launch's stream
  int slot_last;             // ... which is add number slot_last of the slot
  bool wait_barrier;         // behind the newest launch that ran alone (a tile-order refresh, or the tile counters' clearing)
  bool alone;                // refresh or cursor wraps: nobody may still read what this launch rewrites, nobody start on it before
  unsigned wait_streams;     // alone: the other streams whose newest launch it waits for (bit q)
  // afterwards it records: the stream's newest launch, the barrier if alone, the slot's `rendered`
};

// what `stream` waits for when other work joins the pipeline: the last add of every slot that holds a group, the newest launch of streams 1 and up
struct JoinPlan { int n_adds; int slot[PIPE_DEPTH], frame[PIPE_DEPTH]; unsigned streams; };

// group_room: how many frames a group may hold -- the option, if the launch configuration has the builds that store every frame of a batch
// separately (can_store_per_frame), else groups of one
inline int group_room(int pipe_group, bool can_store_per_frame) { return pipe_group <= 1 || !can_store_per_frame ? 1 : pipe_group; }

// Image: a frame's presented picture as the caller gets it (the context: a pinned buffer; the host build: a token).  swap(Image&, Image&) moves one.
template <class Image>
struct TicketBook {
  struct Parked { Image image; bool waited = false; };
  uint64_t next = 0;                               // ticket of the next frame
  uint64_t groups = 0;                             // groups launched so far under this numbering
  int streams = 2;                                 // option pipe_streams when the numbering started (restart_numbering)
  std::vector<HeldFrame> held;                     // tickets [next - size, next)
  SlotBook slot[PIPE_DEPTH];
  // a ticket stays waitable until it has been waited for: when a slot is reused, the images of its frames that were presented and not yet waited
  // for move here (swapped, not copied; their adds have run).  An entry goes at the first launch after its wait
  std::map<uint64_t, Parked> parked;               // by ticket
  bool dirty = false;                              // frames have gone through the pipeline since the last join
  bool last_set[PIPE_STREAMS] = {false, false, false, false};      // the stream has launched a group (its `last` event is recorded)
  bool barrier_set = false;                        // a launch has run alone

  TicketAt locate(uint64_t ticket) const {
    if (ticket < next && ticket + held.size() >= next) return {TICKET_HELD, -1, (int)(ticket + held.size() - next)};
    for (int k = 0; k < PIPE_DEPTH; k++)
      if (slot[k].count > 0 && ticket >= slot[k].first && ticket < slot[k].first + (uint64_t)slot[k].count) return {TICKET_SLOT, k, (int)(ticket - slot[k].first)};
    if (parked.count(ticket)) return {TICKET_PARKED, -1, -1};
    return {ticket >= next ? TICKET_NEVER : TICKET_FINISHED, -1, -1};
  }

  // a group holds frames of ONE view whose seeds are in arithmetic progression (what a progressive render submits): a frame that is neither closes
  // the held group before it is held itself
  bool submit_closes(const float* st13, int W, int H, float bg, uint64_t seed) const {
    if (held.empty()) return false;
    const HeldFrame& p0 = held[0];
    const bool same_view = memcmp(p0.st, st13, sizeof(p0.st)) == 0 && p0.W == W && p0.H == H && p0.bg == bg;
    const bool in_step = held.size() == 1 || seed - held.back().seed == held[1].seed - p0.seed;
    return !same_view || !in_step;
  }
  uint64_t hold(const float* st13, int W, int H, float bg, uint64_t seed, int div) {
    HeldFrame p;
    memcpy(p.st, st13, sizeof(p.st)); p.W = W; p.H = H; p.bg = bg; p.seed = seed; p.div = div;
    held.push_back(p);
    return next++;
  }
  bool group_full(int room) const { return (int)held.size() >= room; }
  // frames of the next launch when the held ones go: all of them as ONE group if a group has the room, else one by one (a defence: whatever
  // shrinks the room launches the held frames before it does)
  int flush_size(int room) const { return room >= (int)held.size() ? (int)held.size() : 1; }
  // ODDITY: the tickets of the frames dropped here wait as finished
  void drop_held() { held.clear(); }

  // images owed to the caller that would be in the store after the next `launches` launches: those in it now and not waited for, and those of the
  // slots these launches reuse
  int owed_after(int launches) const {
    int owed = 0;
    for (const auto& kv : parked) owed += kv.second.waited ? 0 : 1;
    const uint64_t depth = (uint64_t)streams + 1;
    for (int k = 0; k < launches && k < (int)depth; k++) owed += slot[(groups + (uint64_t)k) % depth].unwaited;
    return owed;
  }
  // the refusal: the launch of the group the frame closes and the launch of its own group each reuse a slot; a frame whose launches could leave
  // more than PIPE_PARKED_MAX images owed is not taken, never an image dropped
  bool submit_overfills(bool closes) const { return owed_after(closes ? 2 : 1) > PIPE_PARKED_MAX; }

  // the first n held frames become the next group: parked images that have been waited for were the caller's until now and go
  GroupBegin group_begin(int n) {
    for (auto it = parked.begin(); it != parked.end();) it = it->second.waited ? parked.erase(it) : std::next(it);
    GroupBegin g;
    g.n = n;
    g.slot = (int)(groups % ((uint64_t)streams + 1)); g.stream = (int)(groups % (uint64_t)streams);
    g.first_ticket = next - (uint64_t)held.size();
    g.seed_stride = n > 1 ? held[1].seed - held[0].seed : 0;
    g.n_park = 0;
    const SlotBook& sl = slot[g.slot];
    if (sl.unwaited > 0)
      for (int f = 0; f < sl.count; f++) if (sl.div[f] != 0 && !sl.fwaited[f]) g.park[g.n_park++] = f;
    return g;
  }
  // refresh: the launch recomputes the tile order; cursor_wraps: it clears the tile counters
  GroupPlan group_plan(const GroupBegin& g, bool refresh, bool cursor_wraps) const {
    const SlotBook& sl = slot[g.slot];
    GroupPlan p;
    p.start_behind = !dirty;
    p.host_wait_slot = !sl.drained && sl.count > 0;
    p.stream_wait_slot = sl.count > 0;
    p.slot_last = sl.count - 1;
    p.wait_barrier = barrier_set;
    p.alone = refresh || cursor_wraps;
    p.wait_streams = 0;
    // ODDITY: every stream that has ever launched, also one beyond a pipe_streams that has shrunk since (its event is old: the wait is free)
    if (p.alone) for (int q = 0; q < PIPE_STREAMS; q++) if (q != g.stream && last_set[q]) p.wait_streams |= 1u << q;
    return p;
  }
  // the plan's start_behind is issued: the pipeline's streams hold work until the next join
  void started_behind() { dirty = true; }
  // the plan's waits for the slot are issued (and the host's is over): the slot's previous group gives way.  slot_images: the slot's
  // PIPE_GROUP_MAX images; those of g.park move to the store, the slot keeps what was there in exchange
  void group_take_slot(const GroupBegin& g, Image* slot_images) {
    using std::swap;
    SlotBook& sl = slot[g.slot];
    if (sl.count > 0) sl.drained = true;
    if (sl.unwaited <= 0) return;                  // (the old group's tickets stay where they are until group_commit)
    for (int k = 0; k < g.n_park; k++) {
      Parked& e = parked[sl.first + (uint64_t)g.park[k]];
      swap(e.image, slot_images[g.park[k]]);
      e.waited = false;
    }
    sl.unwaited = 0; sl.count = 0;
  }
  // launched, and its adds and presents enqueued: the slot holds the group, the held frames are gone
  void group_commit(const GroupBegin& g, const GroupPlan& p) {
    SlotBook& sl = slot[g.slot];
    last_set[g.stream] = true;
    if (p.alone) barrier_set = true;
    sl.unwaited = 0;
    for (int f = 0; f < g.n; f++) { sl.div[f] = held[(size_t)f].div; sl.fwaited[f] = false; sl.unwaited += sl.div[f] != 0 ? 1 : 0; }
    sl.first = g.first_ticket; sl.count = g.n; sl.drained = false;
    groups++;
    held.erase(held.begin(), held.begin() + g.n);
  }

  // dr_pipeline_wait has waited for the ticket's add: true when the frame has an image (was presented)
  bool mark_waited(const TicketAt& at, uint64_t ticket) {
    if (at.place == TICKET_PARKED) { parked.find(ticket)->second.waited = true; return true; }
    SlotBook& sl = slot[at.slot];
    const int f = at.frame;
    if (!sl.fwaited[f] && sl.div[f]) sl.unwaited--;
    sl.fwaited[f] = true;
    if (f == sl.count - 1) sl.drained = true;      // (adds run in order: the last one ends the group)
    return sl.div[f] != 0;
  }
  // of a ticket in a slot or parked: dr_pipeline_wait has returned for it; it was presented (a parked one was); its image in the store (null: in its slot)
  bool waited(const TicketAt& at, uint64_t ticket) const { return at.place == TICKET_PARKED ? parked.find(ticket)->second.waited : slot[at.slot].fwaited[at.frame]; }
  bool presented(const TicketAt& at) const { return at.place == TICKET_PARKED || slot[at.slot].div[at.frame] != 0; }
  const Image* parked_image(const TicketAt& at, uint64_t ticket) const { return at.place == TICKET_PARKED ? &parked.find(ticket)->second.image : nullptr; }
  // the host has waited for everything added so far (dr_render_accumulate_pipelined)
  void all_drained() { for (SlotBook& sl : slot) sl.drained = true; }

  // ODDITY: like a launch alone, every slot and stream that was ever used, whatever pipe_streams says now
  JoinPlan join_plan() const {
    JoinPlan j = {0, {0}, {0}, 0};
    if (!dirty) return j;
    for (int k = 0; k < PIPE_DEPTH; k++) if (slot[k].count > 0) { j.slot[j.n_adds] = k; j.frame[j.n_adds++] = slot[k].count - 1; }
    for (int q = 1; q < PIPE_STREAMS; q++) if (last_set[q]) j.streams |= 1u << q;
    return j;
  }
  void joined() { dirty = false; }

  // option pipe_streams changes (the pipeline is drained): slots and streams are numbered by group, so the count starts again, from ticket 0.
  // ODDITY: parked images, owed or not, are forgotten with the old numbering, and tickets held by the caller then name new frames
  void restart_numbering(int new_streams) {
    for (SlotBook& sl : slot) { sl.drained = true; sl.count = 0; sl.unwaited = 0; }
    parked.clear();
    next = 0; groups = 0;
    streams = new_streams;
  }
};

}  // namespace dr
