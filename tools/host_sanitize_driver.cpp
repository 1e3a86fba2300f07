#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "linearise.hpp"
#include "pipeline_state.hpp"
extern "C" {
int dr_scene_load(const char*, const char*, dr_scene**);
void dr_scene_free(dr_scene*);
int dr_scene_build_bvh(dr_scene*, int);
int dr_scene_save_binary(const dr_scene*, const char*);
int dr_scene_load_binary(const char*, dr_scene**);
const char* dr_last_error(void);
}
using namespace dr;

// The pipelined present loop's ticket book (pipeline_state.hpp) through every named scenario of tests/test_pipeline_state_host.py, a frame's image an
// int: what the sanitizers watch is the book's own memory -- the held frames' vector, the parked map across purge and restart, the slots' arrays
namespace {
struct BookReplay {
  TicketBook<int> book;
  int image[PIPE_DEPTH][PIPE_GROUP_MAX] = {{0}};
  int streams = 2, group = 8, token = 1000, bad = 0;
  bool can_store = true, refresh = false, wraps = false;
  GroupBegin g;              // of the last launch
  GroupPlan plan;
  int room() const { return group_room(group, can_store); }
  void expect(bool ok, const char* what) { if (!ok) { printf("pipeline book: %s\n", what); bad++; } }
  void flush(bool fail = false) {
    while (!book.held.empty()) {
      g = book.group_begin(book.flush_size(room()));
      plan = book.group_plan(g, refresh, wraps);
      if (plan.start_behind) book.started_behind();
      book.group_take_slot(g, image[g.slot]);
      if (fail) { book.drop_held(); return; }
      for (int f = 0; f < g.n; f++) if (book.held[(size_t)f].div) image[g.slot][f] = token - (int)book.held.size() + 1 + f;
      book.group_commit(g, plan);
      refresh = wraps = false;
    }
  }
  // -1: refused
  long long submit(int view, uint64_t seed, int div) {
    float st[13] = {(float)view};
    const bool closes = book.submit_closes(st, 96, 64, 0.f, seed);
    if (book.submit_overfills(closes)) return -1;
    if (closes) flush();
    const uint64_t t = book.hold(st, 96, 64, 0.f, seed, div);
    token++;
    if (book.group_full(room())) flush();
    return (long long)t;
  }
  // the image of a waited ticket (0: none)
  int wait(uint64_t ticket) {
    TicketAt at = book.locate(ticket);
    if (at.place == TICKET_HELD) { flush(); at = book.locate(ticket); }
    if (at.place != TICKET_SLOT && at.place != TICKET_PARKED) return 0;
    if (!book.mark_waited(at, ticket)) return 0;
    const int* parked = book.parked_image(at, ticket);
    return parked ? *parked : image[at.slot][at.frame];
  }
  // dr_pipeline_image: the image, or -1 no image of that ticket, -2 the wait comes first, -3 submitted without a present
  int picture(uint64_t ticket) const {
    const TicketAt at = book.locate(ticket);
    if (at.place != TICKET_SLOT && at.place != TICKET_PARKED) return -1;
    if (!book.waited(at, ticket)) return -2;
    if (!book.presented(at)) return -3;
    const int* parked = book.parked_image(at, ticket);
    return parked ? *parked : image[at.slot][at.frame];
  }
  JoinPlan join() { flush(); const JoinPlan j = book.join_plan(); book.joined(); return j; }
  void set_streams(int v) { (void)join(); if (v != streams) book.restart_numbering(v); streams = v; }
  void restart() { set_streams(streams == 2 ? 3 : 2); set_streams(2); group = 8; can_store = true; }      // a fresh numbering under two streams
};

int replay_pipeline_book() {
  BookReplay r, fresh;       // (fresh: 12 and 13 read the streams' flags, which no restart clears)
  // 1-4: a group fills; a view change and a seed out of step close one; a wait launches a held one
  r.group = 3;
  for (int k = 0; k < 3; k++) r.submit(0, 41 + 7 * k, 1);
  r.expect(r.book.groups == 1 && r.book.locate(2).place == TICKET_SLOT && r.g.n == 3 && r.g.seed_stride == 7, "a group of three fills and launches");
  r.submit(0, 1, 1); r.submit(1, 2, 1);
  r.expect(r.book.groups == 2 && r.book.held.size() == 1, "a view change closes the group");
  r.submit(1, 3, 1); r.submit(1, 9, 1);
  r.expect(r.book.groups == 3 && r.book.held.size() == 1, "a seed out of step closes the group");
  r.expect(r.book.locate(6).place == TICKET_HELD && r.wait(6) == 1007 && r.book.locate(6).place == TICKET_SLOT, "a wait launches the held group");
  // 5-9: slots reused with unwaited presents park; an image before its wait is refused, in a slot and parked; a wait returns that ticket's image; a
  // waited entry goes at the next launch and not earlier; a frame without a present whose slot was reused has finished
  r.restart();
  r.group = 1;
  const int base = r.token;
  for (int k = 0; k < 4; k++) r.submit(0, k, k % 2 ? 0 : 1);      // tickets 1 and 3 without a present
  r.expect(r.book.locate(0).place == TICKET_PARKED && r.g.n_park == 1 && r.g.park[0] == 0, "the reused slot's unwaited present parks");
  r.expect(r.picture(0) == -2 && r.picture(2) == -2, "an image asked for before its wait is refused, parked and in a slot");
  r.expect(r.picture(1) == -2 && r.wait(1) == 0 && r.picture(1) == -3 && r.picture(9) == -1, "no image of a frame without a present, nor of a ticket never handed out");
  r.expect(r.wait(0) == base + 1 && r.picture(0) == base + 1, "the parked ticket's own image comes back");
  (void)r.join();
  r.expect(r.book.locate(0).place == TICKET_PARKED, "a waited parked entry stays until a launch");
  r.submit(0, 4, 1);
  r.expect(r.book.locate(0).place == TICKET_FINISHED && r.picture(0) == -1, "the waited entry goes at the next launch");
  r.expect(r.book.locate(1).place == TICKET_FINISHED && r.wait(1) == 0, "a frame without a present whose slot was reused has finished");
  r.submit(0, 5, 1);
  r.expect(r.book.parked.count(2) == 1 && r.book.parked.size() == 1, "the next slot's unwaited present parks");
  // 10: refused at exactly one more than the bound, with one launch and with two (groups of 16: two groups parked, a third unwaited in slot 2)
  r.restart();
  r.group = PIPE_GROUP_MAX;
  for (int k = 0; k < 80; k++) r.expect(r.submit(k / 16 % 2, (uint64_t)(100 * (k / 16) + k % 16), 1) == k, "five groups of 16 are accepted");
  r.expect(r.book.owed_after(0) == 32 && r.book.owed_after(1) == 48 && r.submit(1, 7, 1) == -1, "48 owed after one launch: refused");
  for (uint64_t t = 0; t < 15; t++) (void)r.wait(t);
  r.expect(r.book.owed_after(1) == PIPE_PARKED_MAX + 1 && r.submit(1, 7, 1) == -1, "one launch, 33 owed: refused");
  (void)r.wait(15);
  r.expect(r.book.owed_after(1) == PIPE_PARKED_MAX && r.submit(1, 7, 1) == 80 && r.book.locate(80).place == TICKET_HELD, "one launch, 32 owed: accepted");
  for (uint64_t t = 32; t < 47; t++) (void)r.wait(t);
  r.expect(r.book.owed_after(2) == PIPE_PARKED_MAX + 1 && r.submit(0, 9, 1) == -1, "two launches, 33 owed: the closing frame is refused");
  (void)r.wait(47);
  r.expect(r.book.owed_after(2) == PIPE_PARKED_MAX && r.submit(0, 9, 1) == 81 && r.book.groups == 6, "two launches, 32 owed: accepted, the held group launched");
  // 11: pipe_streams 2 -> 3 -> 4 -> 2 restarts the numbering and forgets parked entries
  for (int v : {3, 4, 2}) {
    r.group = 1;
    for (int k = 0; k < 7; k++) r.submit(0, (uint64_t)k, 1);
    r.expect(!r.book.parked.empty(), "images are parked before the restart");
    r.set_streams(v);
    r.expect(r.book.next == 0 && r.book.groups == 0 && r.book.streams == v && r.book.parked.empty() && r.book.locate(0).place == TICKET_NEVER, "pipe_streams restarts the numbering");
  }
  // 12: the first group after other work starts behind `stream`, later ones do not, until a join
  fresh.group = 1;
  bool behind[3];
  for (int k = 0; k < 3; k++) { fresh.submit(0, (uint64_t)k, 1); behind[k] = fresh.plan.start_behind; }
  fresh.expect(behind[0] && !behind[1] && !behind[2], "only the first group starts behind `stream`");
  JoinPlan j = fresh.join();
  fresh.expect(j.n_adds == 3 && j.streams == 2u && fresh.join().n_adds == 0, "a join waits for every slot's last add and stream 1; a clean pipeline for nothing");
  fresh.submit(0, 5, 1);
  fresh.expect(fresh.plan.start_behind, "after a join the next group starts behind `stream` again");
  // 13: a launch alone waits for every other stream that has launched and records the barrier; the launches after it wait for that barrier
  fresh.set_streams(3);
  fresh.group = 1;
  fresh.submit(0, 1, 1); fresh.submit(0, 2, 1);
  fresh.refresh = true;
  fresh.submit(0, 3, 1);
  fresh.expect(fresh.g.stream == 2 && fresh.plan.alone && fresh.plan.wait_streams == 3u && fresh.book.barrier_set, "a refreshing launch runs alone behind streams 0 and 1");
  fresh.submit(0, 4, 1);
  fresh.expect(fresh.plan.wait_barrier && !fresh.plan.alone && fresh.plan.wait_streams == 0u, "the launch after it waits for the barrier only");
  fresh.wraps = true;
  fresh.submit(0, 5, 1);
  fresh.expect(fresh.g.stream == 1 && fresh.plan.alone && fresh.plan.wait_streams == 5u && fresh.plan.wait_barrier, "a launch that wraps the cursor runs alone too");
  // 14: a failed flush drops the held frames, and their tickets then wait as finished
  r.restart();
  for (int k = 0; k < 3; k++) r.submit(5, (uint64_t)k, 1);
  r.flush(true);
  r.expect(r.book.held.empty() && r.book.locate(0).place == TICKET_FINISHED && r.book.locate(2).place == TICKET_FINISHED && r.wait(1) == 0, "a failed flush drops the held frames: their tickets have finished");
  r.expect(r.submit(5, 9, 1) == 3, "the numbering goes on after a failed flush");
  // 15: groups of one when the configuration cannot store per frame
  r.restart();
  r.can_store = false;
  for (int k = 0; k < 3; k++) { r.submit(0, (uint64_t)k, 1); r.expect(r.book.held.empty() && r.g.n == 1 && r.book.groups == (uint64_t)k + 1, "a group of one per frame"); }
  r.can_store = true;
  for (int k = 3; k < 6; k++) r.submit(0, (uint64_t)k, 1);
  r.can_store = false;       // (the defence in pipeline_flush: held frames the room no longer holds go one by one)
  r.flush();
  r.expect(r.book.groups == 6 && r.g.n == 1, "held frames without the room for a group are launched one by one");
  return r.bad + fresh.bad;
}
}  // namespace

int main(int argc, char** argv) {
  int bad = replay_pipeline_book();
  for (int i = 2; i < argc; i++) {
    dr_scene* s = nullptr;
    int rc = dr_scene_load(argv[i], argv[1], &s);
    if (rc != 0) { printf("%s: load rc %d (%s)\n", argv[i], rc, dr_last_error()); continue; }
    rc = dr_scene_build_bvh(s, 3);
    if (rc != 0) { printf("%s: build rc %d (%s)\n", argv[i], rc, dr_last_error()); dr_scene_free(s); continue; }
    DeviceImage img;
    rc = linearise(s->host, img);
    if (rc != 0) { printf("%s: linearise rc %d (%s)\n", argv[i], rc, dr_last_error()); bad++; }
    rc = dr_scene_save_binary(s, "/tmp/dogeray_asan_x.rtsb");
    dr_scene* t = nullptr;
    if (rc == 0 && dr_scene_load_binary("/tmp/dogeray_asan_x.rtsb", &t) == 0) {
      if (t->host.objects.size() != s->host.objects.size() || memcmp(t->host.bvh.data(), s->host.bvh.data(), s->host.bvh.size() * sizeof(dr_bvh_node)) != 0) { printf("%s: rtsb mismatch\n", argv[i]); bad++; }
      dr_scene_free(t);
    } else { printf("%s: rtsb rc %d (%s)\n", argv[i], rc, dr_last_error()); bad++; }
    // corrupted links must be refused, never followed (miss_node indexed new_id[] unchecked)
    {
      const size_t used = (size_t)s->host.bvh_used, all = s->host.bvh.size();
      struct Mut { size_t node; int field; int value; };
      const Mut muts[] = {{0, 0, (int)all + 7}, {used / 2, 1, -5}, {used - 1, 1, 1 << 30}, {0, 2, -3}, {used / 3, 3, (int)all}, {1, 0, -2}};
      for (const Mut& m : muts) {
        dr_scene bad_scene;
        bad_scene.host = s->host;
        dr_bvh_node& b = bad_scene.host.bvh[m.node < all ? m.node : 0];
        if (m.field == 0) b.hit_node = m.value; else if (m.field == 1) b.miss_node = m.value; else if (m.field == 2) b.children[0] = m.value; else b.children[1] = m.value;
        DeviceImage junk;
        const bool touches = b.active && (m.field < 2 || !b.end);
        if (linearise(bad_scene.host, junk) == 0 && touches) { printf("%s: corrupted link accepted (node %zu field %d)\n", argv[i], m.node, m.field); bad++; }
      }
    }
    printf("%s: ok, %d objects, walk %zu units, wide %zu records depth %d\n", argv[i], s->host.n, img.walk.size(), img.wide.size() / 4, img.wide_depth);
    dr_scene_free(s);
  }
  return bad;
}
