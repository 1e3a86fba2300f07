"""The pipelined present loop's host bookkeeping as it stood before it was folded onto dogeray_amd/csrc/pipeline_state.hpp: class Parent restates,
line for line, the tree of commit d9125f8 --

  context_pipeline.cpp    8-18   join_pipeline: what `stream` waits for
                         46-49   pipeline_group_size
                         52-56   pipeline_slot_of
                         61-69   pipeline_park
                         73-79   pipeline_owed_after
                         82-171  pipeline_flush_some: purge, slot and stream, the waits, the park, alone, the records, the slot's new group
                        180-187  pipeline_flush, and what a failure drops
                        193-228  dr_pipeline_submit
                        230-257  dr_pipeline_wait
                        259-274  dr_pipeline_image
                        276-286  dr_render_accumulate_pipelined
  context.cpp            65-69   flush_held
                         84-91   set_option("pipe_streams")

-- with everything that touches the device left out and what it would have enqueued logged instead: per launch the slot, the stream, the frames, the
first ticket, the seed stride, the frames parked and every wait and record around it.  A present is a token: the integer the caller gave the frame,
so a test can tell whose image comes back.  Written from that tree, not from the header; tests/test_pipeline_state_host.py drives it and the header's
book with the same events.  Tickets and seeds are uint64 as there: the arithmetic wraps."""

M64 = 2 ** 64
PIPE_STREAMS, PIPE_GROUP_MAX = 4, 16
PIPE_DEPTH = PIPE_STREAMS + 1
PIPE_PARKED_MAX = 2 * PIPE_GROUP_MAX
OK, INVALID, DEVICE = 0, -1, -3          # DR_OK, DR_ERR_INVALID, and the code of the failure a test injects


def view_of(v):
    """the integer views of the host build (tools/host_kernel/hk_pipeline.hpp): settings13[0], W, H, background"""
    return (v % 4, 96 + 8 * (v // 8 % 2), 64, v // 4 % 2)


class Slot:
    def __init__(self):
        self.first, self.count, self.unwaited, self.drained = 0, 0, 0, True
        self.div, self.fwaited, self.rgb_host = [0] * PIPE_GROUP_MAX, [False] * PIPE_GROUP_MAX, [0] * PIPE_GROUP_MAX


class Parent:
    """dr_context's pipe_* members and the code around them"""

    def __init__(self):
        self.pipe_streams, self.pipe_group = 2, 8
        self.can_store_per_frame = True      # !pipe_lean && uses_persistent && persistent_can_store_per_frame(...)
        self.pipe_slot = [Slot() for _ in range(PIPE_DEPTH)]
        self.pipe_groups, self.pipe_next = 0, 0
        self.pipe_pending = []               # (view, seed, div, token)
        self.pipe_parked = {}                # ticket -> [rgb, waited]
        self.pipe_last_set, self.pipe_barrier_set, self.pipe_dirty = [False] * PIPE_STREAMS, False, False
        # the world outside the book: what the next launch will find, and what has been enqueued
        self.refresh_due, self.cursor_wraps, self.fail_at = False, False, None
        self.log = []

    # ---- context_pipeline.cpp
    def join_pipeline(self):                                     # 8-18
        if self.pipe_pending:
            rc = self.pipeline_flush()
            if rc != OK: return rc
        if not self.pipe_dirty: return OK
        adds = tuple((k, sl.count - 1) for k, sl in enumerate(self.pipe_slot) if sl.count > 0)
        streams = sum(1 << k for k in range(1, PIPE_STREAMS) if self.pipe_last_set[k])
        self.log.append(("join", adds, streams))
        self.pipe_dirty = False
        return OK

    def pipeline_group_size(self):                               # 46-49
        if self.pipe_group <= 1 or not self.can_store_per_frame: return 1
        return self.pipe_group

    def pipeline_slot_of(self, ticket):                          # 52-56
        for sl in self.pipe_slot:
            if sl.count > 0 and ticket >= sl.first and ticket < sl.first + sl.count: return sl
        return None

    def pipeline_park(self, sl):                                 # 61-69
        parked = []
        for f in range(sl.count):
            if sl.div[f] != 0 and not sl.fwaited[f]:
                e = self.pipe_parked.setdefault(sl.first + f, [0, False])
                e[0], sl.rgb_host[f] = sl.rgb_host[f], e[0]
                e[1] = False
                parked.append(f)
        sl.unwaited = 0; sl.count = 0
        return parked

    def pipeline_owed_after(self, launches):                     # 73-79
        owed = sum(0 if e[1] else 1 for e in self.pipe_parked.values())
        depth = self.pipe_streams + 1
        k = 0
        while k < launches and k < depth:
            owed += self.pipe_slot[(self.pipe_groups + k) % depth].unwaited
            k += 1
        return owed

    def pipeline_flush_some(self, n):                            # 82-171
        for t in [t for t, e in self.pipe_parked.items() if e[1]]: del self.pipe_parked[t]
        first = self.pipe_pending[0]
        stride = (self.pipe_pending[1][1] - first[1]) % M64 if n > 1 else 0
        first_ticket = (self.pipe_next - len(self.pipe_pending)) % M64
        g = self.pipe_groups
        nstreams, depth = self.pipe_streams, self.pipe_streams + 1
        si = g % nstreams
        k = g % depth
        sl = self.pipe_slot[k]
        if self.fail_at == "params": return DEVICE               # make_params
        plan = dict(start_behind=0, host_wait_slot=0, stream_wait_slot=0, slot_last=sl.count - 1, wait_barrier=0, alone=0, wait_streams=0)
        if not self.pipe_dirty:
            plan["start_behind"] = 1
            self.pipe_dirty = True
        if not sl.drained and sl.count > 0:
            plan["host_wait_slot"] = 1
            sl.drained = True
        if sl.count > 0: plan["stream_wait_slot"] = 1
        parked = self.pipeline_park(sl) if sl.unwaited > 0 else []
        if self.fail_at == "grow": return DEVICE                 # sl.frames.grow
        refresh = self.refresh_due
        if self.pipe_barrier_set: plan["wait_barrier"] = 1
        alone = refresh or self.cursor_wraps
        if alone:
            plan["alone"] = 1
            for q in range(PIPE_STREAMS):
                if q != si and self.pipe_last_set[q]: plan["wait_streams"] |= 1 << q
        self.refresh_due = self.cursor_wraps = False             # (the launch has refreshed the order / moved the cursor)
        self.pipe_last_set[si] = True
        if alone: self.pipe_barrier_set = True
        sl.unwaited = 0
        for f in range(n):
            div = self.pipe_pending[f][2]
            sl.div[f] = 0; sl.fwaited[f] = False
            if div != 0:
                sl.rgb_host[f] = self.pipe_pending[f][3]         # launch_present and the copy into the pinned buffer
                sl.div[f] = div
                sl.unwaited += 1
        sl.first = first_ticket; sl.count = n; sl.drained = False
        self.pipe_groups = g + 1
        self.log.append(("launch", k, si, n, first_ticket, stride, tuple(parked), tuple(sorted(plan.items()))))
        del self.pipe_pending[:n]
        return OK

    def pipeline_flush(self):                                    # 180-187
        while self.pipe_pending:
            all_ = len(self.pipe_pending)
            rc = self.pipeline_flush_some(all_ if self.pipeline_group_size() >= all_ else 1)
            if rc != OK:
                self.pipe_pending = []
                return rc
        return OK

    def submit(self, view, seed, div, token):                    # 193-228 -> (rc, ticket)
        closes = False
        if self.pipe_pending:
            p0, pl = self.pipe_pending[0], self.pipe_pending[-1]
            same_view = view_of(p0[0]) == view_of(view)
            in_step = len(self.pipe_pending) == 1 or (seed - pl[1]) % M64 == (self.pipe_pending[1][1] - p0[1]) % M64
            closes = not same_view or not in_step
        if self.pipeline_owed_after(2 if closes else 1) > PIPE_PARKED_MAX: return INVALID, None
        if closes:
            rc = self.pipeline_flush()
            if rc != OK: return rc, None
        self.pipe_pending.append((view, seed, div, token))
        k = self.pipe_next
        self.pipe_next = (k + 1) % M64
        if len(self.pipe_pending) >= self.pipeline_group_size(): return self.pipeline_flush(), k
        return OK, k

    def wait(self, ticket, want_image):                          # 230-257 -> (rc, error text's key, token)
        if ticket < self.pipe_next and (ticket + len(self.pipe_pending)) % M64 >= self.pipe_next:
            rc = self.pipeline_flush()
            if rc != OK: return rc, "flush", None
        sl = self.pipeline_slot_of(ticket)
        if sl is not None:
            f = ticket - sl.first
            if not sl.fwaited[f] and sl.div[f]: sl.unwaited -= 1
            sl.fwaited[f] = True
            if f == sl.count - 1: sl.drained = True
            if want_image:
                if not sl.div[f]: return INVALID, "submitted without a present", None
                return OK, "", sl.rgb_host[f]
            return OK, "", None
        if ticket in self.pipe_parked:
            self.pipe_parked[ticket][1] = True
            return OK, "", self.pipe_parked[ticket][0] if want_image else None
        if ticket >= (self.pipe_next - len(self.pipe_pending)) % M64: return INVALID, "no such ticket", None
        if want_image: return INVALID, "submitted without a present (or released)", None
        return OK, "", None

    def image(self, ticket):                                     # 259-274
        sl = self.pipeline_slot_of(ticket)
        if sl is None:
            if ticket not in self.pipe_parked: return INVALID, "no image of that ticket", None
            if not self.pipe_parked[ticket][1]: return INVALID, "dr_pipeline_wait(ticket) comes first", None
            return OK, "", self.pipe_parked[ticket][0]
        f = ticket - sl.first
        if not sl.fwaited[f]: return INVALID, "dr_pipeline_wait(ticket) comes first", None
        if not sl.div[f]: return INVALID, "submitted without a present", None
        return OK, "", sl.rgb_host[f]

    def accumulate_pipelined(self, view, seed, stride, nframes, token):      # 276-286
        last = 0
        for k in range(nframes):
            rc, last = self.submit(view, (seed + k * stride) % M64, 0, token + k)
            if rc != OK: return rc
        if nframes > 0:
            rc = self.wait(last, False)[0]
            if rc != OK: return rc
            for sl in self.pipe_slot: sl.drained = True
        return OK

    # ---- context.cpp
    def flush_held(self):                                        # 65-69
        if not self.pipe_pending: return OK
        return self.pipeline_flush()

    def set_pipe_streams(self, v):                               # 76, 84-92
        rc = self.flush_held()
        if rc != OK: return rc
        if v != self.pipe_streams:
            if self.join_pipeline() != OK: return DEVICE
            for sl in self.pipe_slot: sl.drained = True; sl.count = 0; sl.unwaited = 0
            self.pipe_parked.clear()
            self.pipe_next = 0; self.pipe_groups = 0
        self.pipe_streams = v
        return OK

    def set_pipe_group(self, v):                                 # 76, 92
        rc = self.flush_held()
        if rc != OK: return rc
        self.pipe_group = v
        return OK

    def set_can_store_per_frame(self, on):                       # 76, 92 of an option the answer depends on (pipe_lean, kernel, occupancy, ...)
        rc = self.flush_held()
        if rc != OK: return rc
        self.can_store_per_frame = on
        return OK

    def dump(self):
        """every member, in the order of the host build's hk_pipeline_dump"""
        w = [self.pipe_next, self.pipe_groups, self.pipe_streams, int(self.pipe_dirty), int(self.pipe_barrier_set)] + [int(s) for s in self.pipe_last_set]
        w.append(len(self.pipe_pending))
        for view, seed, div, _ in self.pipe_pending:
            st0, W, H, bg = view_of(view)
            w += [st0, W, H, bg, seed, div]
        for sl in self.pipe_slot:
            w += [sl.first, sl.count, sl.unwaited, int(sl.drained)] + sl.div + [int(f) for f in sl.fwaited] + sl.rgb_host
        w.append(len(self.pipe_parked))
        for t in sorted(self.pipe_parked):
            w += [t, int(self.pipe_parked[t][1]), self.pipe_parked[t][0]]
        return tuple(v % M64 for v in w)
