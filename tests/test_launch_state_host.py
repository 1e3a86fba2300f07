"""The rules of dogeray_amd/csrc/launch_state.hpp (tile order, camera rays' tile words, sky split), as the host build exports them
(tools/host_kernel.py LaunchState), against a plain restatement of the code they were folded from -- class Parent below, written from the tree before
the fold (commit afd92e3):

  context_render.cpp    50-73    feedback_buffers: the order an own-site launch may use, the key it stores
                        80-122   cert_prepare: reuse / skip (held) / skip (first sight) / compute, and the key of 22 floats
                        131-154  sky_split: the key of five words, "room and key match"
                        171-176  enqueue_frame, the hold_order arm
                        188-196  enqueue_frame after the launch: age, refresh rhythm, generation
  context_pipeline.cpp  129-137  the launch that refreshes runs alone: the rhythm's factor 4
  context.cpp           90-93    set_option: which options drop which cache
  launch_plan.hpp       256-259  order_geometry: five floats, stripe and regions packed into one

Both are driven by the same events and must take the same decisions and hold the same state after every event: hand-written sequences that walk
every arm, then seeded random ones over a small alphabet -- two settings vectors x two geometries, scene uploads, batch 1 or 8, held / own / pipelined
site, the options on and off, a wide walk or not, a view that gives words or not -- and every arm must have been reached by the random part.  The
typed keys are compared through the parent's packing (the scene generation modulo 2^24 as there: the one intended difference, never reached).  No GPU."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

F = np.float32
SETTINGS = (np.arange(13, dtype=F) + F(0.5), np.arange(13, dtype=F) * F(2.0) - F(3.0))
# W, H, stripe mod, stripe rem, ncols, gy, regions -- 64 tiles in one queue, 128 tiles of a stripe in eight
GEOMETRIES = ((64, 64, 1, 0, 8, 8, 1), (256, 128, 2, 1, 16, 8, 8))


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


def order_geometry(g):
    """launch_plan.hpp 256-259"""
    W, H, mod, rem, ncols, gy, regions = g
    return np.array([F(W), F(H), F(mod * 1024 + rem) + F(0.125) * F(regions), F(ncols), F(gy)], F)


class Options:
    def __init__(self):
        self.feedback, self.order_follows_camera, self.feedback_every = 1, 1, 8
        self.camera_cert, self.camera_entry, self.cert_factor, self.cert_levels, self.sky_tiles = 1, 1, 40, 1, 2
        self.scene_gen, self.own_bounds, self.wide = 1, True, True


class Parent:
    """dr_context's loose members and the code around them, as they were"""

    def __init__(self):
        self.order_valid, self.order_capacity, self.order_age, self.order_gen = False, 0, 0, 0
        self.order_key = np.zeros(18, F)
        self.cert_valid = self.cert_ok = self.entry_ok = False
        self.cert_key, self.cert_seen, self.cert_tiles, self.cert_gen = np.zeros(22, F), np.zeros(22, F), 0, 0
        self.sky_key, self.sky_key_valid, self.sky_split_last, self.sky_room = (0, 0, 0, 0, 0), False, False, 0

    def set_option(self, reorders, drops_words):          # context.cpp 90-93
        if drops_words: self.cert_valid = False
        if reorders: self.order_valid = False

    def pipeline_refresh(self, o, g, tiles):              # context_pipeline.cpp 129-137
        refresh = False
        if o.feedback and tiles > 0:
            refresh = (not self.order_valid or self.order_capacity < tiles or not np.array_equal(self.order_key[13:], order_geometry(g)) or self.order_age < 2 or
                       self.order_age % (4 * o.feedback_every) == 0)
        return refresh

    def launch(self, o, st, g, batch, hold, view_ok, plan_splits):
        """enqueue_frame's persistent arm -> (order used, costs recorded, words plan, words read, split, split reused, feedback pass)"""
        tiles, regions = g[4] * g[5], g[6]
        if hold:                                          # context_render.cpp 171-176
            order = self.order_valid and self.order_capacity >= tiles and np.array_equal(self.order_key[13:], order_geometry(g))
            pcost = False
        else:                                             # feedback_buffers, 50-73
            order = pcost = False
            if o.feedback:
                if self.order_capacity < tiles:
                    self.order_capacity = 0; self.order_valid = False
                    self.order_capacity = tiles
                key = np.concatenate([st, order_geometry(g)])
                if self.order_valid and np.array_equal(self.order_key, key): order = True
                elif self.order_valid and o.order_follows_camera and np.array_equal(self.order_key[13:], key[13:]):
                    order = True
                    self.order_key = key
                    self.order_age = 0
                else: self.order_key = key; self.order_valid = False
                pcost = True
        # cert_prepare, 80-122
        plan, reads = "not wanted", False
        want_cert = bool(o.camera_cert and o.own_bounds)
        want_entry = bool(o.camera_entry)
        if (want_cert or want_entry) and o.wide and tiles > 0:
            W, H, mod, rem, ncols, gy, _ = g
            key = np.concatenate([st, np.array([W, H, mod, rem, ncols, gy, o.scene_gen & 0xffffff, o.cert_factor, o.cert_levels + 2 * o.camera_entry + 4 * o.camera_cert], F)])
            plan = "reuse"
            if not (self.cert_valid and np.array_equal(self.cert_key, key)):
                if hold: plan = "skip: held"
                elif batch < 2 and not np.array_equal(self.cert_seen, key): self.cert_seen = key; plan = "skip: first sight"
                else:
                    plan = "compute"
                    self.cert_valid = False
                    self.cert_ok = self.entry_ok = False
                    self.cert_gen += 1
                    if view_ok: self.cert_ok, self.entry_ok = want_cert, want_entry
                    self.cert_key = key
                    self.cert_tiles = tiles
                    self.cert_valid = True
            if plan in ("reuse", "compute"): reads = self.cert_ok or self.entry_ok
        # sky_split, 131-154
        split = bool(o.sky_tiles and self.entry_ok and reads and not hold and plan_splits)
        reused = False
        if split:
            key = (self.cert_gen, 1 if order else 0, self.order_gen if order else 0, tiles, regions)
            reused = self.sky_room >= tiles and self.sky_key_valid and self.sky_key == key
            if not reused:
                self.sky_room = max(self.sky_room, tiles)
                self.sky_key, self.sky_key_valid = key, True
        self.sky_split_last = split
        # after the launch, 188-196
        if pcost and not order: self.order_age = 0
        refresh = bool(pcost and (self.order_age < 2 or self.order_age % o.feedback_every == 0))
        if refresh:
            self.order_gen += 1
            self.order_valid = True
        self.order_age += 1
        return bool(order), pcost, plan, bool(reads), split, bool(reused), refresh

    def read_backs(self, o):                              # context.cpp: a certificate / an entry table can be read back (without the buffers' checks)
        return (bool(o.camera_cert and self.cert_valid and self.cert_ok and self.cert_tiles > 0), bool(o.camera_entry and self.cert_valid and self.entry_ok and self.cert_tiles > 0))


class Folded:
    """the same launch through the exported rules, as context_render.cpp now asks them"""

    def __init__(self, hk):
        self.s = hk.LaunchState()
        self.sky_room = 0

    @staticmethod
    def view(o, st, g):
        return st, dict(W=g[0], H=g[1], stripe_mod=g[2], stripe_rem=g[3], ncols=g[4], gy=g[5], regions=g[6], scene_gen=o.scene_gen, cert_factor=o.cert_factor,
                        cert_levels=o.cert_levels, camera_entry=o.camera_entry, camera_cert=o.camera_cert)

    def set_option(self, reorders, drops_words):
        self.s.invalidate(order=reorders, words=drops_words)

    def pipeline_refresh(self, o, g, tiles):
        return bool(o.feedback and tiles > 0 and self.s.order_pipeline_refresh(self.view(o, SETTINGS[0], g), tiles, o.feedback_every))

    def launch(self, o, st, g, batch, hold, view_ok, plan_splits):
        tiles, regions = g[4] * g[5], g[6]
        v = self.view(o, st, g)
        use = self.s.order_begin(v, tiles, o.feedback, o.order_follows_camera, hold)
        want_cert, want_entry = bool(o.camera_cert and o.own_bounds), bool(o.camera_entry)
        plan = self.s.camera_words_plan(v, want_cert, want_entry, o.wide, tiles, hold, batch)
        if plan == "compute": self.s.camera_words_compute(v, tiles, want_cert and view_ok, want_entry and view_ok)
        reads = plan in ("reuse", "compute") and self.s.camera_words_readable()[2]
        split = bool(o.sky_tiles and self.s.read()["words"]["entry_ok"] and reads and not hold and plan_splits)
        reused = self.s.sky_split_launch(split, use[0], tiles, regions, self.sky_room >= tiles)
        if split and not reused: self.sky_room = max(self.sky_room, tiles)
        refresh = self.s.order_end(use, o.feedback_every)
        return use[0], use[1], plan, bool(reads), split, reused, refresh

    def read_backs(self, o):
        r = self.s.camera_words_readable()
        return bool(o.camera_cert and r[0]), bool(o.camera_entry and r[1])


def _bits(a):
    return tuple(int(v) for v in np.asarray(a, F).view(np.uint32))


def _packed(key, words):
    """a typed key (settings13's words, KEY_FIELDS' values) in the parent's packing: 18 floats of the order's key, or 22 of the words'"""
    st, (W, H, mod, rem, ncols, gy, regions, gen, factor, levels, entry, cert) = key
    tail = [W, H, mod, rem, ncols, gy, gen & 0xffffff, factor, levels + 2 * entry + 4 * cert] if words else list(order_geometry((W, H, mod, rem, ncols, gy, regions)))
    return st + _bits(np.array(tail, F))


def assert_same_state(p, f, where):
    s = f.s.read()
    o, w, k = s["order"], s["words"], s["sky"]
    assert (o["valid"], o["capacity"], o["age"], o["gen"]) == (int(p.order_valid), p.order_capacity, p.order_age, p.order_gen), where
    assert _packed(o["key"], False) == _bits(p.order_key), where
    assert (w["valid"], w["cert_ok"], w["entry_ok"], w["tiles"], w["gen"]) == (int(p.cert_valid), int(p.cert_ok), int(p.entry_ok), p.cert_tiles, p.cert_gen), where
    assert _packed(w["key"], True) == _bits(p.cert_key) and _packed(w["seen"], True) == _bits(p.cert_seen), where
    assert (k["valid"], k["last"]) == (int(p.sky_key_valid), int(p.sky_split_last)), where
    assert (k["words_gen"], k["ordered"], k["order_gen"], k["tiles"], k["regions"]) == p.sky_key, where


class Pair:
    """the two sides under the same events; `arms` counts what was reached"""

    def __init__(self, hk, arms):
        self.o, self.p, self.f, self.arms, self.n = Options(), Parent(), Folded(hk), arms, 0

    def reach(self, arm):
        self.arms[arm] = self.arms.get(arm, 0) + 1

    def check(self, what):
        self.n += 1
        assert_same_state(self.p, self.f, (self.n, what))
        a, b = self.p.read_backs(self.o), self.f.read_backs(self.o)
        assert a == b, (self.n, what, a, b)
        self.reach("certificate readable" if a[0] else "no certificate to read"); self.reach("table readable" if a[1] else "no table to read")

    def option(self, name, value):
        setattr(self.o, name, value)
        reorders, drops_words = name in ("feedback", "heavy_factor"), name in ("camera_cert", "camera_entry", "cert_factor", "cert_levels", "sky_tiles")
        self.p.set_option(reorders, drops_words); self.f.set_option(reorders, drops_words)
        self.reach("option drops the order" if reorders else "option drops the words" if drops_words else "option drops nothing")
        self.check(("option", name, value))

    def upload(self, own_bounds):
        self.o.scene_gen += 1; self.o.own_bounds = own_bounds
        self.check("upload")

    def launch(self, v, g, batch, site, view_ok=True, plan_splits=True):
        st, geo = SETTINGS[v], GEOMETRIES[g]
        tiles = geo[4] * geo[5]
        hold = site == "held"
        if site == "pipelined":
            a, b = self.p.pipeline_refresh(self.o, geo, tiles), self.f.pipeline_refresh(self.o, geo, tiles)
            assert a == b, (self.n, "pipeline", a, b)
            if a:
                stale = not self.p.order_valid or self.p.order_capacity < tiles or not np.array_equal(self.p.order_key[13:], order_geometry(geo))
                self.reach("pipeline: refresh, the order does not serve" if stale else "pipeline: refresh, the rhythm")
            else: self.reach("pipeline: hold")
            hold, plan_splits = not a, False          # (per-frame stores are not split)
        before = (self.p.order_valid, self.p.order_capacity, self.p.order_age)
        full = np.array_equal(self.p.order_key, np.concatenate([st, order_geometry(geo)]))          # (tells the two arms that use the order apart)
        a = self.p.launch(self.o, st, geo, batch, hold, view_ok, plan_splits)
        b = self.f.launch(self.o, st, geo, batch, hold, view_ok, plan_splits)
        assert a == b, (self.n, "launch", v, g, batch, site, a, b)
        order, pcost, plan, reads, split, reused, refresh = a
        if hold: self.reach("held: the order serves" if order else "held: no order")
        elif not self.o.feedback: self.reach("own: no feedback")
        else:
            if before[1] < tiles: self.reach("own: the buffers grow")
            self.reach("own: full match" if order and full else "own: follows the camera" if order else "own: mismatch")
        self.reach("words: " + plan)
        if plan == "compute": self.reach("compute: the view gives words" if view_ok else "compute: the view gives none")
        if plan == "not wanted": self.reach("not wanted: no wide walk" if not self.o.wide else "not wanted: the options")
        self.reach("sky: not split" if not split else "sky: reused" if reused else "sky: split anew")
        self.reach("after: feedback pass" if refresh else "after: no pass")
        if pcost and not order: self.reach("after: age reset")
        self.check(("launch", v, g, batch, site))
        return a


ARMS = ("held: the order serves", "held: no order", "own: no feedback", "own: the buffers grow", "own: full match", "own: follows the camera", "own: mismatch",
        "after: feedback pass", "after: no pass", "after: age reset", "pipeline: refresh, the order does not serve", "pipeline: refresh, the rhythm", "pipeline: hold",
        "words: not wanted", "words: reuse", "words: skip: held", "words: skip: first sight", "words: compute", "compute: the view gives words",
        "compute: the view gives none", "not wanted: no wide walk", "not wanted: the options", "sky: not split", "sky: reused", "sky: split anew",
        "certificate readable", "no certificate to read", "table readable", "no table to read", "option drops the order", "option drops the words",
        "option drops nothing")


def test_hand_written_sequences_walk_every_arm(hk):
    arms = {}
    p = Pair(hk, arms)
    # (order used, costs recorded, words plan, words read, split, split reused, feedback pass)
    assert p.launch(0, 0, 8, "own") == (False, True, "compute", True, True, False, True)          # mismatch, the buffers grow, age reset; split anew
    assert p.launch(0, 0, 8, "own") == (True, True, "reuse", True, True, False, True)             # full match; second launch of the view refreshes; the order is new to the split
    assert p.launch(0, 0, 8, "own") == (True, True, "reuse", True, True, False, False)            # age 2: no pass; the order's generation moved: split anew
    assert p.launch(0, 0, 8, "own") == (True, True, "reuse", True, True, True, False)             # ... and now reused
    assert p.launch(1, 0, 1, "own") == (True, True, "skip: first sight", False, False, False, True)      # follows the camera: age 0, refreshed at once
    assert p.launch(1, 0, 1, "own") == (True, True, "compute", True, True, False, True)           # the view's second launch computes
    for k in range(2, 9):
        assert p.launch(1, 0, 1, "own")[6] == (k == 8), k                                         # the rhythm: every 8th
    assert p.launch(1, 0, 8, "held") == (True, False, "reuse", True, False, False, False)         # held: reads order and words, records nothing
    assert p.launch(1, 1, 8, "held") == (False, False, "skip: held", False, False, False, False)  # other geometry, and more tiles than the buffers hold
    p.option("order_follows_camera", 0)
    assert p.launch(0, 0, 8, "own")[:3] == (False, True, "compute")                               # mismatch where the camera is not followed
    p.option("feedback", 0)
    assert p.launch(0, 0, 8, "own")[:2] == (False, False) and p.launch(0, 0, 8, "held")[:2] == (False, False)
    p.option("feedback", 1)
    assert p.launch(0, 0, 8, "pipelined")[:2] == (False, True)                                    # no order: the launch refreshes, alone
    assert p.launch(0, 0, 8, "pipelined")[:2] == (True, True)                                     # age 1: again
    for k in range(2, 33):
        got = p.launch(0, 0, 8, "pipelined")
        assert got[:2] == ((True, True) if k == 32 else (True, False)) and got[6] == (k == 32), k  # held until four times the rhythm
    p.option("camera_entry", 0); p.option("camera_cert", 0)
    assert p.launch(0, 0, 8, "own")[2:5] == ("not wanted", False, False)
    p.option("camera_entry", 1); p.option("camera_cert", 1)
    assert p.launch(0, 0, 8, "own")[2] == "compute"                                               # the option dropped the words
    assert p.launch(0, 0, 8, "own", view_ok=True)[2] == "reuse"
    p.upload(own_bounds=False)
    assert p.launch(0, 0, 8, "own", view_ok=False)[:5] == (True, True, "compute", False, False)   # the order survives the upload, the words do not; no words for this view
    assert p.launch(0, 0, 8, "own")[2:4] == ("reuse", False)                                      # ... which is remembered
    p.option("camera_entry", 0)
    assert p.launch(0, 0, 8, "own")[2] == "not wanted"                                            # no own bounds, no table wanted
    p.option("camera_entry", 1)
    p.o.wide = False
    assert p.launch(0, 0, 8, "own")[2] == "not wanted"
    p.o.wide = True
    p.upload(own_bounds=True)
    p.option("sky_tiles", 0)
    assert p.launch(0, 1, 8, "own")[2:5] == ("compute", True, False)
    p.option("sky_tiles", 2)
    assert p.launch(0, 1, 8, "own", plan_splits=False)[4] is False
    p.option("heavy_factor", 0)
    assert p.launch(0, 1, 8, "own")[0] is False
    missing = [a for a in ARMS if a not in arms]
    assert not missing, missing


def test_random_sequences_agree_and_reach_every_arm(hk):
    rng = random.Random(20240607)
    arms = {}
    events = 0
    for _ in range(2500):
        p = Pair(hk, arms)
        for _ in range(24):
            r = rng.random()
            if r < 0.70:
                p.launch(rng.randrange(2), 0 if rng.random() < 0.7 else 1, rng.choice((1, 1, 8)), rng.choice(("own", "own", "held", "pipelined", "pipelined")),
                        view_ok=rng.random() < 0.85, plan_splits=rng.random() < 0.8)
            elif r < 0.78: p.upload(own_bounds=rng.random() < 0.5)
            elif r < 0.80: p.o.wide = not p.o.wide
            else:
                name = rng.choice(("feedback", "order_follows_camera", "camera_cert", "camera_entry", "cert_levels", "sky_tiles", "heavy_factor", "feedback_every"))
                p.option(name, {"feedback_every": rng.choice((1, 2, 8)), "sky_tiles": rng.randrange(3), "heavy_factor": rng.randrange(2)}.get(name, 1 - getattr(p.o, name, 0)))
            events += 1
    print("%d events; arms reached: %s" % (events, sorted(arms.items())))
    missing = [a for a in ARMS if a not in arms]
    assert not missing, missing
