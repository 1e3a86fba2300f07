"""The pipelined present loop's bookkeeping (dogeray_amd/csrc/pipeline_state.hpp: the ticket book, locate, the rules that close and size a group, the
ordering plans), as the host build exports it (tools/host_kernel.py PipelineBook, a frame's image an integer token), against tests/pipeline_walk.py --
a restatement of the code it was folded from.  Both are driven by the same events and after EVERY event must agree on four things: the result (return
code, error, ticket), the launches and joins issued (slot, stream, frames, first ticket, seed stride, frames parked, the whole ordering plan), the token
handed back, and a dump of the whole book.  Class Folded is context_pipeline.cpp / context.cpp after the fold, without the device: it only asks the book.

Named scenarios first, each asserted to reach its case; then seeded random sequences over 2 .. 4 streams and groups of 1 .. 16; last a few direct
assertions with hand-computed answers, which stand without the restatement.  No GPU."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

import pipeline_walk as walk      # noqa: E402
from pipeline_walk import DEVICE, INVALID, OK      # noqa: E402

STRIDE = 1000003


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


class Folded:
    """the entry points as they now read, over the exported book"""

    def __init__(self, hk):
        self.b = hk.PipelineBook()
        self.pipe_streams, self.pipe_group, self.can_store_per_frame = 2, 8, True
        self.refresh_due, self.cursor_wraps, self.fail_at = False, False, None
        self.tokens = []                     # of the held frames (the pixels a present would make)
        self.log = []

    def held(self):
        return len(self.tokens)

    def join_pipeline(self):
        if self.held():
            rc = self.pipeline_flush()
            if rc != OK: return rc
        before = self.b.dump()[3]            # (dirty: a join of a clean pipeline enqueues nothing)
        adds, streams = self.b.join()
        if before: self.log.append(("join", adds, streams))
        return OK

    def group_room(self):
        return self.hk_room(self.pipe_group, self.can_store_per_frame)

    def pipeline_flush_some(self, n):
        slot, stream, first, stride, parked = self.b.group_begin(n)
        if self.fail_at == "params": return DEVICE
        plan = self.b.group_plan(self.refresh_due, self.cursor_wraps)
        self.b.group_take_slot()
        if self.fail_at == "grow": return DEVICE
        self.refresh_due = self.cursor_wraps = False
        self.b.group_commit(self.tokens[:n])
        del self.tokens[:n]
        self.log.append(("launch", slot, stream, n, first, stride, parked, tuple(sorted(plan.items()))))
        return OK

    def pipeline_flush(self):
        while self.held():
            rc = self.pipeline_flush_some(self.b.flush_size(self.group_room()))
            if rc != OK:
                self.b.drop_held(); self.tokens = []
                return rc
        return OK

    def submit(self, view, seed, div, token):
        closes = self.b.submit_closes(view, seed)
        if self.b.submit_overfills(closes): return INVALID, None
        if closes:
            rc = self.pipeline_flush()
            if rc != OK: return rc, None
        k = self.b.hold(view, seed, div)
        self.tokens.append(token)
        if self.b.group_full(self.group_room()): return self.pipeline_flush(), k
        return OK, k

    def wait(self, ticket, want_image):
        at = self.b.locate(ticket)
        if at[0] == "held":
            rc = self.pipeline_flush()
            if rc != OK: return rc, "flush", None
            at = self.b.locate(ticket)
        if at[0] == "slot":
            presented = self.b.mark_waited(ticket)
            if want_image:
                if not presented: return INVALID, "submitted without a present", None
                return OK, "", self.b.image(ticket)
            return OK, "", None
        if at[0] == "parked":
            self.b.mark_waited(ticket)
            return OK, "", self.b.image(ticket) if want_image else None
        if at[0] == "finished":
            if want_image: return INVALID, "submitted without a present (or released)", None
            return OK, "", None
        return INVALID, "no such ticket", None

    def image(self, ticket):
        place, _, _, waited, presented = self.b.locate(ticket)
        if place not in ("slot", "parked"): return INVALID, "no image of that ticket", None
        if not waited: return INVALID, "dr_pipeline_wait(ticket) comes first", None
        if not presented: return INVALID, "submitted without a present", None
        return OK, "", self.b.image(ticket)

    def accumulate_pipelined(self, view, seed, stride, nframes, token):
        last = 0
        for k in range(nframes):
            rc, last = self.submit(view, (seed + k * stride) % walk.M64, 0, token + k)
            if rc != OK: return rc
        if nframes > 0:
            rc = self.wait(last, False)[0]
            if rc != OK: return rc
            self.b.all_drained()
        return OK

    def flush_held(self):
        return self.pipeline_flush() if self.held() else OK

    def set_pipe_streams(self, v):
        rc = self.flush_held()
        if rc != OK: return rc
        if v != self.pipe_streams:
            if self.join_pipeline() != OK: return DEVICE
            self.b.restart_numbering(v)
        self.pipe_streams = v
        return OK

    def set_pipe_group(self, v):
        rc = self.flush_held()
        if rc != OK: return rc
        self.pipe_group = v
        return OK

    def set_can_store_per_frame(self, on):
        rc = self.flush_held()
        if rc != OK: return rc
        self.can_store_per_frame = on
        return OK


class Pair:
    """the two sides under the same events; every event is compared in full"""

    def __init__(self, hk, reached=None):
        self.p, self.f = walk.Parent(), Folded(hk)
        self.f.hk_room = lambda group, can: hk.lib().hk_pipeline_group_room(group, int(can))
        self.reached = {} if reached is None else reached
        self.n, self.token = 0, 1000
        self.launches = []                   # of the last event

    def reach(self, what):
        self.reached[what] = self.reached.get(what, 0) + 1

    def both(self, what, call, world=None):
        """runs call(side) on both sides; returns the parent's result"""
        self.n += 1
        for side in (self.p, self.f):
            side.log = []
            if world: world(side)
        a, b = call(self.p), call(self.f)
        where = (self.n, what)
        assert a == b, (where, a, b)
        assert self.p.log == self.f.log, (where, self.p.log, self.f.log)
        assert (self.p.refresh_due, self.p.cursor_wraps) == (self.f.refresh_due, self.f.cursor_wraps), where
        da, db = self.p.dump(), self.f.b.dump()
        assert da == db, (where, [(i, x, y) for i, (x, y) in enumerate(zip(da, db)) if x != y][:8], len(da), len(db))
        assert len(self.p.pipe_pending) == self.f.held(), where
        self.launches = [e for e in self.p.log if e[0] == "launch"]
        for e in self.launches:
            plan = dict(e[7])
            self.reach("launch of %s" % ("one" if e[3] == 1 else "several"))
            if e[6]: self.reach("frames park")
            if plan["start_behind"]: self.reach("starts behind `stream`")
            if plan["host_wait_slot"]: self.reach("host waits for the slot")
            if plan["stream_wait_slot"] and not plan["host_wait_slot"]: self.reach("slot drained already")
            if plan["alone"]: self.reach("alone" if plan["wait_streams"] else "alone, nobody to wait for")
            if plan["wait_barrier"]: self.reach("waits for the barrier")
        if any(e[0] == "join" for e in self.p.log): self.reach("join")
        return a

    def submit(self, view, seed, div=1):
        self.token += 1
        t = self.token
        rc, ticket = self.both(("submit", view, seed, div), lambda s: s.submit(view, seed, div, t))
        self.reach("submit refused" if rc == INVALID else "submit fails" if rc != OK else "submit")
        return rc, ticket, t

    def wait(self, ticket, want_image=True):
        r = self.both(("wait", ticket, want_image), lambda s: s.wait(ticket, want_image))
        self.reach("wait: " + (r[1] or "ok"))
        return r

    def image(self, ticket):
        r = self.both(("image", ticket), lambda s: s.image(ticket))
        self.reach("image: " + (r[1] or "ok"))
        return r

    def flush(self, fail_at=None):
        """an option or an upload arrives; fail_at: the launch it causes fails in make_params ("params") or when the slot's buffers grow ("grow")"""
        def world(s): s.fail_at = fail_at
        rc = self.both(("flush", fail_at), lambda s: s.flush_held(), world)
        for s in (self.p, self.f): s.fail_at = None
        if rc != OK: self.reach("flush fails at " + fail_at)
        return rc

    def join(self):
        return self.both("join", lambda s: s.join_pipeline())

    def set_streams(self, v):
        return self.both(("pipe_streams", v), lambda s: s.set_pipe_streams(v))

    def set_group(self, v):
        return self.both(("pipe_group", v), lambda s: s.set_pipe_group(v))

    def set_can_store(self, on):
        return self.both(("can store per frame", on), lambda s: s.set_can_store_per_frame(on))

    def refresh_due(self):
        def world(s): s.refresh_due = True
        self.both("refresh due", lambda s: OK, world)

    def cursor_wraps(self):
        def world(s): s.cursor_wraps = True
        self.both("cursor wraps", lambda s: OK, world)

    def batch(self, view, seed, n):
        self.token += n
        t = self.token - n + 1
        return self.both(("batch", view, seed, n), lambda s: s.accumulate_pipelined(view, seed, STRIDE, n, t))

    def place(self, ticket):
        return self.f.b.locate(ticket)[0]


def seeds(n, first=41):
    return [first + k * STRIDE for k in range(n)]


def launch_fields(e):
    """(slot, stream, frames, first ticket, stride, parked) and the plan of a logged launch"""
    return e[1:7], dict(e[7])


def test_a_group_fills_and_launches_itself(hk):
    p = Pair(hk)
    p.set_group(3)
    for k, s in enumerate(seeds(3)):
        rc, ticket, _ = p.submit(0, s)
        assert (rc, ticket) == (OK, k)
        assert len(p.launches) == (1 if k == 2 else 0)
    fields, plan = launch_fields(p.launches[0])
    assert fields == (0, 0, 3, 0, STRIDE, ())
    assert plan == dict(start_behind=1, host_wait_slot=0, stream_wait_slot=0, slot_last=-1, wait_barrier=0, alone=0, wait_streams=0)
    assert [p.place(t) for t in range(4)] == ["slot"] * 3 + ["never"]


def test_a_view_change_closes_a_group(hk):
    p = Pair(hk)
    p.submit(0, 41); p.submit(0, 41 + STRIDE)
    assert not p.launches
    p.submit(1, 41 + 2 * STRIDE)             # in step, but another view
    assert [launch_fields(e)[0] for e in p.launches] == [(0, 0, 2, 0, STRIDE, ())]
    assert p.place(1) == "slot" and p.place(2) == "held"
    for other in (4, 8):                     # the background, the frame size
        p.submit(other, 7)
        assert len(p.launches) == 1


def test_a_seed_out_of_step_closes_a_group(hk):
    p = Pair(hk)
    p.submit(0, 41); p.submit(0, 41 + STRIDE); p.submit(0, 41 + 2 * STRIDE)
    assert not p.launches
    p.submit(0, 41 + 4 * STRIDE)
    assert [launch_fields(e)[0] for e in p.launches] == [(0, 0, 3, 0, STRIDE, ())]
    p.submit(0, 41 + 4 * STRIDE - 5)         # a stride of -5 (it wraps) is a progression too: two frames always are
    assert not p.launches
    p.flush()
    assert launch_fields(p.launches[0])[0] == (1, 1, 2, 3, walk.M64 - 5, ())


def test_a_wait_for_a_held_ticket_launches_its_group(hk):
    p = Pair(hk)
    tokens = [p.submit(0, s)[2] for s in seeds(3)]
    assert p.place(1) == "held" and not p.launches
    assert p.wait(1) == (OK, "", tokens[1])
    assert [launch_fields(e)[0] for e in p.launches] == [(0, 0, 3, 0, STRIDE, ())]
    assert p.place(1) == "slot"


def park_three(p):
    """groups of one under two streams: tickets 0 .. 2 fill the three slots, ticket 3 reuses slot 0 and parks ticket 0; the tokens"""
    p.set_group(1)
    tokens = [p.submit(0, s, div=k + 1)[2] for k, s in enumerate(seeds(4))]
    fields, plan = launch_fields(p.launches[0])
    assert fields == (0, 1, 1, 3, 0, (0,)) and plan["host_wait_slot"] and plan["stream_wait_slot"] and plan["slot_last"] == 0
    assert p.place(0) == "parked" and p.place(3) == "slot"
    return tokens


def test_a_reused_slot_parks_its_unwaited_presents_and_a_wait_returns_that_tickets_image(hk):
    p = Pair(hk)
    tokens = park_three(p)
    assert p.wait(0) == (OK, "", tokens[0])
    assert p.wait(3) == (OK, "", tokens[3])
    assert p.image(0) == (OK, "", tokens[0]) and p.image(3) == (OK, "", tokens[3])


def test_an_image_asked_for_before_its_wait_is_refused_in_a_slot_and_parked(hk):
    p = Pair(hk)
    park_three(p)
    assert p.place(0) == "parked" and p.image(0) == (INVALID, "dr_pipeline_wait(ticket) comes first", None)
    assert p.place(2) == "slot" and p.image(2) == (INVALID, "dr_pipeline_wait(ticket) comes first", None)
    assert p.image(4) == (INVALID, "no image of that ticket", None)


def test_a_waited_parked_entry_goes_at_the_next_launch_and_not_earlier(hk):
    p = Pair(hk)
    tokens = park_three(p)
    p.wait(0)
    p.join(); p.wait(1); p.image(0)          # nothing but a launch releases it
    assert p.place(0) == "parked" and p.image(0) == (OK, "", tokens[0])
    p.submit(0, 5, div=9)                    # the launch of ticket 4 (slot 1: ticket 1 was waited for, nothing parks)
    assert launch_fields(p.launches[0])[0] == (1, 0, 1, 4, 0, ())
    assert p.place(0) == "finished"
    assert p.image(0) == (INVALID, "no image of that ticket", None)
    assert p.wait(0) == (INVALID, "submitted without a present (or released)", None) and p.wait(0, False) == (OK, "", None)


def test_a_frame_without_a_present_whose_slot_was_reused_waits_as_finished(hk):
    p = Pair(hk)
    p.set_group(1)
    for s in seeds(4): p.submit(0, s, div=0)
    assert launch_fields(p.launches[0])[0] == (0, 1, 1, 3, 0, ())      # slot 0 again, nothing parked
    assert p.place(0) == "finished"
    assert p.wait(0, False) == (OK, "", None)
    assert p.wait(0, True) == (INVALID, "submitted without a present (or released)", None)
    assert p.wait(1, True) == (INVALID, "submitted without a present", None)          # still in its slot: the other text
    assert p.wait(9, False) == (INVALID, "no such ticket", None)


@pytest.mark.parametrize("closes", [False, True])
def test_a_submit_is_refused_at_exactly_one_more_than_the_bound(hk, closes):
    """PIPE_PARKED_MAX images may be owed after the launches a submit can cause: one launch if the frame joins or fills a group, two if it closes one
    (the held group's launch and its own).  Groups of 16 under two streams: two groups parked are 32 owed, and slot 2 holds a third, unwaited group."""
    p = Pair(hk)
    p.set_group(16)
    n = 0
    for g in range(5):                       # five full groups: slots 0, 1, 2, then 0 and 1 again park 32 images
        for k in range(16):
            assert p.submit(g % 2, 100 * g + k)[0] == OK
            n += 1
    def owed(launches):                      # both sides' count
        a, b = p.p.pipeline_owed_after(launches), p.f.b.owed_after(launches)
        assert a == b, (launches, a, b)
        return a

    assert owed(0) == 32 and owed(1) == 48 and p.p.pipe_groups == 5
    # the next launch reuses slot 2 (16 unwaited): 48 > 32, every submit is refused ...
    assert p.submit(1, 7)[0] == INVALID
    # ... until enough is waited for: after 15 waits in the store 17 + 16 = 33 are owed after one launch -- exactly one more than the bound
    for t in range(15): assert p.wait(t)[0] == OK
    assert owed(1) == 33 == p.f.b.PARKED_MAX + 1
    if not closes:
        assert not p.f.held() and p.submit(1, 7)[0] == INVALID      # no group held, the frame closes nothing: its one launch counts, 33
        assert p.p.pipe_next == 80                                  # (a refused submit takes no ticket)
    # ... and after the 16th 16 + 16 = 32: at the bound
    assert p.wait(15)[0] == OK
    assert owed(1) == 32 and owed(2) == 48
    if not closes:
        rc, ticket, _ = p.submit(1, 7)       # accepted at exactly the bound; no group held: one launch counts
        assert (rc, ticket) == (OK, 80) and p.place(80) == "held"
        assert p.submit(1, 8)[0] == OK       # joins the group: still one launch, 32
        assert p.submit(0, 9)[0] == INVALID  # closes it: two launches, slots 2 and 0 -- 16 + 16 + 16 = 48
        p.wait(32)                           # one image of slot 2 less: 47, still too many
        assert p.submit(0, 9)[0] == INVALID
    else:
        for t in range(32, 47): p.wait(t)    # slot 2 keeps one unwaited frame: one launch 16 + 1 = 17, two launches 16 + 1 + 16 = 33
        assert owed(1) == 17 and owed(2) == 33
        assert p.submit(1, 7)[0] == OK       # held
        assert p.submit(0, 9)[0] == INVALID  # would close it: 33 = PIPE_PARKED_MAX + 1
        p.wait(47)
        assert owed(2) == 32
        rc, ticket, _ = p.submit(0, 9)       # 32: at the bound, accepted
        assert (rc, ticket) == (OK, 81) and len(p.launches) == 1
    assert p.reached["submit refused"] >= 2


def test_pipe_streams_restarts_the_numbering_and_forgets_parked_entries(hk):
    p = Pair(hk)
    park_three(p)
    for v in (3, 4, 2):
        assert p.f.b.dump()[0] > 0
        assert p.set_streams(v) == OK
        d = p.f.b.dump()
        assert d[:3] == (0, 0, v) and d[-1] == 0, d[:3]         # next ticket, groups, streams; nothing parked
        assert p.place(0) == "never"
        tickets = [p.submit(0, s, div=1)[1] for s in seeds(v + 2)]
        assert tickets == list(range(v + 2))
        assert p.place(0) == "parked"                           # v + 1 slots: ticket v + 1 took ticket 0's
        assert launch_fields(p.launches[0])[0][:2] == (0, (v + 1) % v)
    assert p.set_streams(2) == OK and p.f.b.dump()[0] > 0       # the same value: nothing restarts


def test_the_first_group_after_other_work_starts_behind_stream_until_a_join(hk):
    p = Pair(hk)
    p.set_group(1)
    plans = []
    for s in seeds(3):
        p.submit(0, s)
        plans.append(launch_fields(p.launches[0])[1]["start_behind"])
    assert plans == [1, 0, 0]
    p.join()
    assert p.p.log == [("join", ((0, 0), (1, 0), (2, 0)), 0b10)]      # every slot's last add, stream 1's newest launch (stream 0 is `stream` itself)
    p.join()
    assert p.p.log == []                     # clean: nothing to wait for
    p.submit(0, 5)
    assert launch_fields(p.launches[0])[1]["start_behind"] == 1


def test_a_launch_alone_waits_for_the_other_streams_and_the_later_ones_for_its_barrier(hk):
    p = Pair(hk)
    p.set_streams(3); p.set_group(1)
    p.submit(0, 1); p.submit(0, 2)           # streams 0 and 1 have launched, 2 has not
    p.refresh_due()
    p.submit(0, 3)
    fields, plan = launch_fields(p.launches[0])
    assert fields[:2] == (2, 2) and plan["alone"] and plan["wait_streams"] == 0b011 and not plan["wait_barrier"]
    p.submit(0, 4)
    plan = launch_fields(p.launches[0])[1]
    assert plan["wait_barrier"] and not plan["alone"] and plan["wait_streams"] == 0
    p.cursor_wraps()
    p.submit(0, 5)
    fields, plan = launch_fields(p.launches[0])
    assert fields[:2] == (0, 1) and plan["alone"] and plan["wait_streams"] == 0b101 and plan["wait_barrier"]


def test_a_failed_flush_drops_the_held_frames_and_their_tickets_wait_as_finished(hk):
    for where in ("params", "grow"):
        p = Pair(hk)
        tickets = [p.submit(0, s)[1] for s in seeds(3)]
        assert p.flush(fail_at=where) == DEVICE
        assert not p.launches and p.f.held() == 0
        assert [p.place(t) for t in tickets] == ["finished"] * 3      # ODDITY (kept): never rendered, and a wait says OK
        assert p.wait(tickets[0], False) == (OK, "", None)
        assert p.submit(0, 7)[1] == 3        # the numbering goes on
    # a failure where the buffers grow comes after the slot was taken: its old group has parked by then
    p = Pair(hk)
    tokens = park_three(p)
    p.set_group(8)
    p.submit(0, 1); p.submit(0, 2)           # tickets 4, 5 held; the next launch takes slot 1 (ticket 1, unwaited)
    assert p.flush(fail_at="grow") == DEVICE
    assert p.place(1) == "parked" and p.wait(1) == (OK, "", tokens[1])


def test_groups_of_one_form_when_the_configuration_cannot_store_per_frame(hk):
    p = Pair(hk)
    assert p.set_can_store(False) == OK
    for k, s in enumerate(seeds(3)):
        p.submit(0, s)
        assert [launch_fields(e)[0][2:4] for e in p.launches] == [(1, k)]
    p.set_can_store(True)
    for s in seeds(3): p.submit(0, s)
    assert not p.launches and p.f.held() == 3
    p.set_can_store(False)                   # the change launches what is held first, as one group
    assert [launch_fields(e)[0][2] for e in p.launches] == [3]
    # the defence in pipeline_flush: held frames that the room no longer holds go one by one (no entry point leaves them held across the change)
    p.set_can_store(True)
    for s in seeds(3): p.submit(0, s)
    p.p.can_store_per_frame = p.f.can_store_per_frame = False
    p.flush()
    assert [launch_fields(e)[0][2] for e in p.launches] == [1, 1, 1]


def test_a_pipelined_batch_leaves_every_slot_drained(hk):
    p = Pair(hk)
    assert p.batch(0, 41, 20) == OK
    assert [e[3] for e in p.launches] == [8, 8, 4]
    p.submit(0, 5)
    p.flush()
    assert not launch_fields(p.launches[0])[1]["host_wait_slot"] and launch_fields(p.launches[0])[1]["stream_wait_slot"]


def test_random_sequences_show_no_difference(hk):
    rng = random.Random(20241021)
    reached = {}
    events = 0
    for q in range(240):
        p = Pair(hk, reached)
        p.set_streams(2 + q % 3)
        p.set_group(rng.choice((1, 1, 2, 3, 5, 8, 16, rng.randrange(1, 17))))
        view, seed, stride = 0, rng.randrange(1000), rng.choice((1, STRIDE))
        handed = []                          # tickets handed out under the current numbering
        for _ in range(320):
            r = rng.random()
            if r < 0.50:
                if rng.random() < 0.12: view = rng.randrange(16)
                if rng.random() < 0.05: seed = rng.randrange(walk.M64)      # out of step (and now and then across the wrap)
                seed = (seed + stride) % walk.M64
                rc, ticket, _ = p.submit(view, seed, div=rng.choice((0, 1, 1, 2, 7)))
                if rc == OK: handed.append(ticket)
            elif r < 0.72:
                t = rng.choice(handed[-40:]) if handed and rng.random() < 0.9 else rng.randrange(0, 400)
                p.wait(t, rng.random() < 0.7)
            elif r < 0.80: p.image(rng.choice(handed[-40:]) if handed and rng.random() < 0.9 else rng.randrange(0, 400))
            elif r < 0.84: p.flush()
            elif r < 0.855: p.flush(fail_at=rng.choice(("params", "grow")))
            elif r < 0.87:
                v = rng.randrange(2, 5)
                if v != p.p.pipe_streams: handed = []
                p.set_streams(v)
            elif r < 0.89: p.set_group(rng.randrange(1, 17))
            elif r < 0.90: p.set_can_store(rng.random() < 0.6)
            elif r < 0.93: p.refresh_due()
            elif r < 0.95: p.cursor_wraps()
            elif r < 0.99: p.join()
            else: p.batch(view, rng.randrange(1000), rng.randrange(0, 20))
        events += p.n
    print("%d events; reached: %s" % (events, sorted(reached.items())))
    want = ("launch of one", "launch of several", "frames park", "starts behind `stream`", "host waits for the slot", "slot drained already", "alone",
            "alone, nobody to wait for", "waits for the barrier", "join", "submit", "submit refused", "wait: ok", "wait: submitted without a present",
            "wait: submitted without a present (or released)", "wait: no such ticket", "image: ok", "image: no image of that ticket",
            "image: dr_pipeline_wait(ticket) comes first", "image: submitted without a present", "flush fails at params", "flush fails at grow")
    missing = [w for w in want if w not in reached]
    assert not missing, missing


def test_locate_and_owed_after_by_hand(hk):
    """no restatement here: a book driven directly, the answers worked out by hand.  Three streams, groups of 2: slot = group % 4, stream = group % 3"""
    b = hk.PipelineBook()
    assert hk.lib().hk_pipeline_parked_max() == 32
    assert [hk.lib().hk_pipeline_group_room(g, c) for g, c in ((8, 1), (8, 0), (1, 1), (16, 1), (0, 1))] == [8, 1, 1, 16, 1]
    b.restart_numbering(3)

    def group(div):
        for k in range(2): b.hold(0, b.dump()[0], div)
        begin = b.group_begin(2)
        b.group_plan(False, False); b.group_take_slot(); b.group_commit([500 + begin[2], 501 + begin[2]])
        return begin

    assert b.locate(0)[0] == "never" and b.owed_after(1) == 0
    assert group(1) == (0, 0, 0, 1, ())      # tickets 0, 1 -> slot 0, stream 0; the seeds are the tickets: stride 1
    assert group(0) == (1, 1, 2, 1, ())      # 2, 3 -> slot 1, not presented
    assert group(1) == (2, 2, 4, 1, ())      # 4, 5 -> slot 2
    assert group(1) == (3, 0, 6, 1, ())      # 6, 7 -> slot 3
    b.hold(0, 99, 1)                         # ticket 8, held
    assert [b.locate(t)[:3] for t in (0, 3, 5, 8, 9)] == [("slot", 0, 0), ("slot", 1, 1), ("slot", 2, 1), ("held", -1, 0), ("never", -1, -1)]
    # the next launches reuse slots 0, 1, 2, 3: 2 owed, then 2 + 0, then 2 + 0 + 2, then 8 -- and never more than the four slots there are
    assert [b.owed_after(n) for n in (0, 1, 2, 3, 4, 9)] == [0, 2, 2, 4, 6, 6]
    b.mark_waited(1)
    assert [b.owed_after(n) for n in (1, 4)] == [1, 5]
    begin = b.group_begin(1)
    assert begin == (0, 1, 8, 0, (0,))       # group 4 -> slot 0, stream 1; of tickets 0 and 1 only 0 is still owed
    b.group_plan(False, False); b.group_take_slot(); b.group_commit([508])
    assert b.locate(0)[0] == "parked" and b.image(0) == 500 and b.locate(1)[0] == "finished" and b.locate(8)[:3] == ("slot", 0, 0)
    assert [b.owed_after(n) for n in (0, 1, 2)] == [1, 1, 3]            # ticket 0 parked; slot 1 owes nothing, slot 2 two
