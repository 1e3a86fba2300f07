"""The lane patterns of tests/test_gpu_store_merged.py and tests/test_merge_cases_host.py, and the reference they are judged by: what the stores of a
batched launch (dogeray_amd/csrc/device_shade.hpp store_pixel, store_pixels_merged, store_pixels_merged_lds) must leave in the accumulator when the
caller, not the renderer, says which lanes of a wave store which pixel under which key in the same phase (dr_kat_store_merged).

A case (one per class, built once from SEED and never changed) is a list of waves of exactly 64 lanes and is ONE call of the hook.  Wave w owns the
columns [w * band, (w + 1) * band) of an accumulator H = 5 rows high and the keys [w * 4096, (w + 1) * 4096) -- counted down from 2^31 in the class
of large keys --, so a wrong pixel names its wave, and one key never names two pixels of the call (the hook refuses that).  Only "across_waves"
lets every wave store into the same two pixels.  A lane that does not store carries the wave's decoy pixel (the last of its band, which nothing stores
into) and, every other lane, a key of a storing lane: a merge that let such a lane take part shows in the decoy or in a sum.  The LDS rows a wave
starts with are random words unless a class says otherwise: no form may read what it did not write.

The reference has no slots, no leaders and no order: the three integers each storing lane adds (the oracle's kat_store of the lane's colour) are added
per pixel in int64 to the initial accumulator, and the sums wrapped to int32.  Every class states the property it was made for as a function of its
inputs (CLASSES, check_property), so that none passes for want of the pattern."""
import numpy as np

I32, I64, F32 = np.int32, np.int64, np.float32
SEED = 20260
H = 5
KEYS_PER_WAVE = 4096
ROWS = 7                                             # LDS rows of a wave: a guard, the five slot rows (key, lane, three sums), a guard
ROW_KEY, ROW_LANE, ROW_SUMS = 1, 2, (3, 4, 5)
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31
GUARD = 0x6A5D0000                                   # guard word of column c: GUARD + c (row 0), ~(GUARD + c) (row 6)
BIG = 1e30                                           # a colour beyond int32: the conversion saturates


def wrap32(a):
    """int64 -> the int32 with the same low 32 bits"""
    return (np.asarray(a, I64) & I64(0xFFFFFFFF)).astype(np.uint32).view(I32)


class Case:
    """One call: store_me, key, x, y int32[waves, 64]; color float32[waves, 64, 3]; lds_in int32[waves, 7, 64]; acc int32[W, H, 3]"""

    def __init__(self, name, rng, band=3, spp=1, keys_down=False, shared=False):
        self.name, self.rng, self.band, self.spp, self.keys_down, self.shared = name, rng, band, spp, keys_down, shared
        self.waves = []

    # -- building
    def key(self, w, local):
        assert 0 <= local < KEYS_PER_WAVE
        w = 0 if self.shared else w
        return 2 ** 31 - KEYS_PER_WAVE * (w + 1) + local if self.keys_down else KEYS_PER_WAVE * w + local

    def pixel(self, w, p):
        assert 0 <= p < self.band * H
        return (0 if self.shared else w) * self.band + p // H, p % H

    def wave(self, groups, colours=None, lds=None):
        """groups: (local key, local pixel, lanes) each; colours: float32[64, 3] (default: ordinary random colours); lds: int32[7, 64] or a function
        of (this wave's keys int32[64], its mask) that returns them (default: random words between the guards)"""
        w = len(self.waves)
        store = np.zeros(64, I32)
        key = np.zeros(64, I32)
        x, y = np.zeros(64, I32), np.zeros(64, I32)
        decoy = self.band * H - 1
        for local, p, lanes in groups:
            lanes = np.asarray(list(lanes), np.int64)
            assert p != decoy and not store[lanes].any(), "a lane in two groups, or a group on the decoy"
            store[lanes] = 1
            key[lanes] = self.key(w, local)
            x[lanes], y[lanes] = self.pixel(w, p)
        idle = np.flatnonzero(store == 0)
        used = np.unique(key[store != 0])
        for n, lane in enumerate(idle):
            key[lane] = used[n // 2 % len(used)] if len(used) and n % 2 == 0 else self.key(w, int(self.rng.integers(0, KEYS_PER_WAVE)))
            x[lane], y[lane] = self.pixel(w, decoy)
        if colours is None:
            colours = self.rng.uniform(0, 4, (64, 3)).astype(F32)
        rows = random_rows(self.rng)
        if callable(lds):
            rows = lds(rows, key, store != 0)
        elif lds is not None:
            rows = np.array(lds, I32)
        assert rows.shape == (ROWS, 64) and np.asarray(colours).shape == (64, 3)
        self.waves.append((store, key, x, y, np.asarray(colours, F32), rows))
        return self

    def finish(self, acc=None):
        st, key, x, y, col, lds = (np.ascontiguousarray(np.stack(a)) for a in zip(*self.waves))
        self.store_me, self.key_, self.x, self.y, self.color, self.lds_in = st, key, x, y, col, lds
        self.n_waves = len(self.waves)
        self.W = self.band * (1 if self.shared else self.n_waves)
        self.acc = self.rng.integers(-100000, 100000, (self.W, H, 3)).astype(I32) if acc is None else acc(self)
        for a in (self.store_me, self.key_, self.x, self.y, self.color, self.lds_in, self.acc):
            a.flags.writeable = False
        del self.waves, self.rng
        return self

    # -- reading
    @property
    def mask(self):
        return self.store_me != 0

    @property
    def slot(self):
        return self.key_ & 63

    def lanes(self, first=0, last=None):
        """the hook's lane arrays, flat, for the waves [first, last): store_me, key, x, y, color"""
        s = slice(first, last)
        return (self.store_me[s].reshape(-1), self.key_[s].reshape(-1), self.x[s].reshape(-1), self.y[s].reshape(-1), self.color[s].reshape(-1, 3))


def random_rows(rng):
    rows = rng.integers(INT32_MIN, INT32_MAX, (ROWS, 64), dtype=np.int64).astype(I32)
    rows[0] = GUARD + np.arange(64)
    rows[ROWS - 1] = ~(GUARD + np.arange(64))
    return rows


# ------------------------------------------------------------------ the reference, and a second formulation of it
def lane_integers(case, kat_store):
    """int32[waves, 64, 3]: what a store of each lane's colour adds -- kat_store(color float32[n, 3], spp) -> int32[n, 3], the oracle's"""
    return np.asarray(kat_store(case.color.reshape(-1, 3), case.spp), I32).reshape(case.n_waves, 64, 3)


def sums64(case, ints, first=0, last=None):
    """the accumulator plus the storing lanes' integers of waves [first, last), per pixel, in int64: not wrapped"""
    s = slice(first, last)
    acc = case.acc.astype(I64)
    m = case.mask[s]
    np.add.at(acc, (case.x[s][m], case.y[s][m]), ints[s][m].astype(I64))
    return acc


def reference(case, ints, first=0, last=None):
    return wrap32(sums64(case, ints, first, last))


def reference_naive(case, ints):
    """one lane after the other, wrapped to int32 after every add"""
    acc = [int(v) for v in case.acc.reshape(-1)]
    for w in range(case.n_waves):
        for lane in range(64):
            if case.store_me[w, lane]:
                at = (int(case.x[w, lane]) * H + int(case.y[w, lane])) * 3
                for ch in range(3):
                    acc[at + ch] = (acc[at + ch] + int(ints[w, lane, ch]) + 2 ** 31) % 2 ** 32 - 2 ** 31
    return np.array(acc, I64).astype(I32).reshape(case.acc.shape)


def untouched_slots(case):
    """bool[waves, 64]: the slots of a wave that no storing lane's key addresses -- form 2 leaves their five words alone"""
    out = np.ones((case.n_waves, 64), bool)
    for w in range(case.n_waves):
        out[w, case.slot[w][case.mask[w]]] = False
    return out


# ------------------------------------------------------------------ properties (of the inputs alone)
def collision_pairs(case, w):
    """pairs of storing lanes of wave w with the same slot and different keys"""
    m = case.mask[w]
    k, s = case.key_[w][m].astype(I64), case.slot[w][m]
    return int(((s[:, None] == s[None, :]) & (k[:, None] != k[None, :])).sum()) // 2


def groups_on_collided_slots(case, w):
    """the sizes of the key groups of wave w that share their slot with another key: [[sizes on one slot], ...]"""
    m = case.mask[w]
    out = []
    for s in np.unique(case.slot[w][m]):
        keys, counts = np.unique(case.key_[w][m & (case.slot[w] == s)], return_counts=True)
        if len(keys) > 1:
            out.append(counts.tolist())
    return out


def every_loser_group_has_lanes(case, w):
    """a collision whose losers have more than one lane whichever key wins the slot: on some collided slot every group has at least two lanes"""
    return any(min(sizes) >= 2 for sizes in groups_on_collided_slots(case, w))


def leaves_int32(case, ints):
    s = sums64(case, ints)
    return bool(((s > INT32_MAX) | (s < INT32_MIN)).any())


def prop_one_pixel(case, ints):
    for w in range(case.n_waves):
        assert case.mask[w].any() and len(np.unique(case.key_[w][case.mask[w]])) == 1, w
    assert sorted(case.mask.sum(axis=1).tolist()) == sorted([64, 1, 2, 31, 32, 33, 63] + [1, 2, 31, 32, 33, 63])


def prop_one_lane(case, ints):
    assert [np.flatnonzero(m).tolist() for m in case.mask] == [[p] for p in (0, 1, 15, 16, 31, 32, 47, 48, 63)]


def prop_no_lane(case, ints):
    assert not case.mask.any() and case.n_waves >= 1
    assert np.array_equal(reference(case, ints), case.acc)


def prop_order0_like(case, ints):
    for w in range(case.n_waves):
        assert case.mask[w].all() and len(np.unique(case.slot[w])) == 64 and collision_pairs(case, w) == 0
        assert len(set(zip(case.x[w].tolist(), case.y[w].tolist()))) == 64


def prop_split_pixels(case, ints):
    sizes = []
    for w in range(case.n_waves):
        assert case.mask[w].all() and collision_pairs(case, w) == 0
        keys, counts = np.unique(case.key_[w], return_counts=True)
        assert len(np.unique(keys & 63)) == len(keys) > 1
        sizes.append(sorted(counts.tolist()))
    assert sizes.count([32, 32]) == 2 and sizes.count([1, 63]) == 2 and sizes.count([16, 16, 16, 16]) == 2
    # both assignments: a wave whose groups are runs of lanes, and one whose neighbouring lanes all differ
    changes = [(np.diff(case.key_[w]) != 0).sum() for w in range(case.n_waves)]
    assert min(changes) == 1 and max(changes) == 63


def prop_collisions(case, ints):
    for w in range(case.n_waves):
        assert collision_pairs(case, w) >= 1, w
    sizes = [sorted(map(sorted, groups_on_collided_slots(case, w))) for w in range(case.n_waves)]
    assert sizes.count([[1, 63]]) >= 2 and sizes.count([[32, 32]]) >= 2, "k against k + 64 in both proportions and both lane orders"
    assert any(len(s) == 1 and len(s[0]) == 3 for s in sizes), "three keys on one slot"
    assert [[1] * 64] in sizes, "64 keys on one slot"
    assert any(len(s) == 2 for s in sizes), "two collided slots in one wave"
    # either group can be the one that wins the slot, whichever lane's write stays: the lone lane is the wave's highest in one wave and its lowest in
    # another, and of two halves the lower key holds the highest lane in one wave and the lowest in another
    ends = set()
    for w in range(case.n_waves):
        k = case.key_[w]
        if sizes[w] == [[1, 63]]:
            ends.add(("lone lane", int((k == k[63]).sum()), int((k == k[0]).sum())))
        if sizes[w] == [[32, 32]]:
            ends.add(("halves", bool(k[63] < k[0]), bool(k[0] < k[63])))
    assert ends >= {("lone lane", 1, 63), ("lone lane", 63, 1), ("halves", True, False), ("halves", False, True)}, ends


def prop_large_keys(case, ints):
    for w in range(case.n_waves):
        assert collision_pairs(case, w) >= 1, w
    k = case.key_[case.mask].astype(I64)
    assert k.max() >= 2 ** 31 - 64 and k.min() >= 2 ** 31 - KEYS_PER_WAVE * case.n_waves


def prop_slot_vs_lane(case, ints):
    lane = np.arange(64)
    seen = set()
    for w in range(case.n_waves):
        m, s, k = case.mask[w], case.slot[w], case.key_[w]
        if m[63] and s[63] == 0: seen.add("slot 0 from lane 63")
        if m[0] and s[0] == 63: seen.add("slot 63 from lane 0")
        for l in lane[m]:
            if s[l] != l and (m & (s == l) & (k != k[l])).any(): seen.add("a lane whose own slot index holds another pixel")
            if not m[s[l]]: seen.add("a slot whose lane does not store")
    assert len(seen) == 4, seen


def prop_wraps(case, ints):
    assert leaves_int32(case, ints)
    for w in range(case.n_waves):      # ... in every wave's own pixels
        cols = slice(w * case.band, (w + 1) * case.band)
        s = sums64(case, ints, w, w + 1)[cols]
        assert ((s > INT32_MAX) | (s < INT32_MIN)).any(), w


def prop_values(case, ints):
    c = case.color[case.mask]
    assert np.isnan(c).any() and np.isposinf(c).any() and np.isneginf(c).any() and (c < 0).any()
    v = ints[case.mask]
    assert (v == INT32_MAX).any() and (v == INT32_MIN).any() and (v < 0).any()
    assert leaves_int32(case, ints)


def prop_stale(case, ints):
    kinds = set()
    for w in range(case.n_waves):
        m, s, k, rows = case.mask[w], case.slot[w], case.key_[w], case.lds_in[w]
        assert m.any()
        addressed = np.unique(s[m])
        if all(rows[ROW_KEY, a] in k[m & (s == a)] for a in addressed): kinds.add("the key row holds a key about to be written")
        if all(rows[ROW_KEY, a] not in k[m] and rows[ROW_KEY, a] & 63 == a and rows[ROW_KEY, a] >= 0 for a in addressed): kinds.add("the key row holds a colliding key")
        if all(0 <= rows[ROW_LANE, a] < 64 for a in addressed):
            kinds.add("the lane row holds lane numbers")
            if all(m[rows[ROW_LANE, a]] for a in addressed): kinds.add("... of storing lanes")
        assert all((rows[r, addressed] != 0).all() for r in ROW_SUMS), "sum rows non-zero"
        assert np.array_equal(rows[0], GUARD + np.arange(64)) and np.array_equal(rows[ROWS - 1], ~(GUARD + np.arange(64)))
    assert len(kinds) == 4, kinds
    assert any(collision_pairs(case, w) >= 1 for w in range(case.n_waves)) and any(collision_pairs(case, w) == 0 for w in range(case.n_waves))


def prop_across_waves(case, ints):
    assert case.n_waves == 64 and case.mask.all()
    assert len(set(zip(case.x.reshape(-1).tolist(), case.y.reshape(-1).tolist()))) == 2 and len(np.unique(case.key_)) == 2


FUZZ_KINDS = ("no collision", "a collision with a loser group of more than one lane", "an empty mask", "a full mask")


def fuzz_kinds(case):
    """kind -> the share of the waves that are of it (a wave can be of several)"""
    n = {k: 0 for k in FUZZ_KINDS}
    for w in range(case.n_waves):
        m = case.mask[w]
        n["no collision"] += m.any() and collision_pairs(case, w) == 0
        n["a collision with a loser group of more than one lane"] += every_loser_group_has_lanes(case, w)
        n["an empty mask"] += not m.any()
        n["a full mask"] += m.all()
    return {k: v / case.n_waves for k, v in n.items()}


def prop_fuzz(case, ints):
    assert case.n_waves == 256
    shares = fuzz_kinds(case)
    assert min(shares.values()) >= 0.10, shares
    keys = np.unique(case.key_[case.mask] % KEYS_PER_WAVE)
    slots = (keys & 63).tolist()
    assert len(keys) == 6 and sorted(slots.count(s) for s in set(slots)) == [1, 1, 2, 2], "six pixels, two pairs on one slot each"
    assert np.isnan(case.color[case.mask]).any() and (ints[case.mask] == INT32_MAX).any()


# ------------------------------------------------------------------ the classes
def special_colours():
    import shade_cases as sc
    return sc.store_colours()


def pool_colours(rng, n=64, special=0.25):
    """ordinary colours with a share of rows of shade_cases.store_colours() (NaN, infinities, beyond int32 either way, negative) among them"""
    pool = special_colours()
    c = rng.uniform(0, 4, (n, 3)).astype(F32)
    pick = rng.random(n) < special
    c[pick] = pool[rng.integers(0, len(pool) - 1000, int(pick.sum()))]      # (the pool's last 1000 rows are ordinary)
    return c


def build_one_pixel(c):
    c.wave([(5, 0, range(64))])
    for n in (1, 2, 31, 32, 33, 63):
        c.wave([(7 + n, n % 14, range(n))])                                                # the first n lanes
        c.wave([(70 + n, (n + 3) % 14, sorted(c.rng.permutation(64)[:n].tolist()))])      # any n lanes
    return c.finish()


def build_one_lane(c):
    for p in (0, 1, 15, 16, 31, 32, 47, 48, 63):
        c.wave([(100 + p, p % 14, [p])])
    return c.finish()


def build_no_lane(c):
    return c.wave([]).wave([]).finish()


def build_order0_like(c):
    for _ in range(2):
        slots = c.rng.permutation(64)
        c.wave([(int(s) + 64 * int(c.rng.integers(0, 64)), lane, [lane]) for lane, s in enumerate(slots)])
    return c.finish()


def build_split_pixels(c):
    lanes = np.arange(64)
    c.wave([(3, 0, lanes[:32]), (4, 1, lanes[32:])])
    c.wave([(3, 0, lanes[lanes % 2 == 0]), (4, 1, lanes[lanes % 2 == 1])])
    c.wave([(10, 2, [0]), (11, 3, lanes[1:])])
    c.wave([(10, 2, [37]), (11, 3, lanes[lanes != 37])])
    c.wave([(20 + g, 4 + g, lanes[16 * g:16 * g + 16]) for g in range(4)])
    c.wave([(20 + g, 4 + g, lanes[lanes % 4 == g]) for g in range(4)])
    return c.finish()


def collision_waves(c, k=9, step=64):
    lanes = np.arange(64)
    for a, b in ((k, k + step), (k + step, k)):                         # both lane orders: the key of the low lanes, the key of the high lanes
        c.wave([(a, 0, [0]), (b, 1, lanes[1:])])
        c.wave([(a, 0, lanes[:63]), (b, 1, [63])])
        c.wave([(a, 0, lanes[:32]), (b, 1, lanes[32:])])
        c.wave([(a, 0, lanes[lanes % 2 == 0]), (b, 1, lanes[lanes % 2 == 1])])
    c.wave([(k, 0, lanes[lanes % 3 == 0]), (k + step, 1, lanes[lanes % 3 == 1]), (k + 2 * step, 2, lanes[lanes % 3 == 2])])
    c.wave([(k, 0, lanes[:20]), (k + step, 1, lanes[20:40]), (k + 2 * step, 2, lanes[40:])])
    return c


def build_collisions(c):
    lanes = np.arange(64)
    collision_waves(c)
    order = c.rng.permutation(64)
    c.wave([(33 + 64 * int(j), lane, [lane]) for lane, j in enumerate(order)])          # 64 keys on slot 33: one winner, 63 lone losers
    c.wave([(2, 0, lanes[:16]), (2 + 64, 1, lanes[16:32]), (50, 2, lanes[32:48]), (50 + 192, 3, lanes[48:])])      # two slots, a collision on each
    c.wave([(2, 0, lanes[lanes % 4 == 0]), (2 + 64, 1, lanes[lanes % 4 == 3]), (50, 2, lanes[lanes % 4 == 1]), (50 + 192, 3, lanes[lanes % 4 == 2])])
    return c.finish()


def build_large_keys(c):
    return collision_waves(c, KEYS_PER_WAVE - 64 + 9, -64).finish()      # wave 0: 2^31 - 64 + 9 against 2^31 - 128 + 9


def build_slot_vs_lane(c):
    lanes = np.arange(64)
    c.wave([(64 * 3 + 0, 0, [63])])                                  # slot 0 from lane 63 alone: slot - lane = -63
    c.wave([(64 * 5 + 63, 1, [0])])                                  # slot 63 from lane 0 alone: + 63
    c.wave([(0, 0, [63, 62]), (63, 1, [0, 1]), (64, 2, [30])])
    # lanes 7 and 8 store pixel A (slot 40); pixel B's key has slot 7 and is stored by lanes 40, 41 -- each group's slot is the other's lane, all four store
    c.wave([(40, 0, [7, 8]), (64 + 7, 1, [40, 41])])
    # the slot's own lane (12) stores nothing; with a collision on it
    c.wave([(12, 0, [3, 4, 5]), (12 + 64, 1, [50, 51])])
    # every lane stores the slot of its mirror lane: 64 pixels, slot - lane from -63 to 63
    c.wave([(63 - lane + 64 * (lane % 5), lane, [lane]) for lane in lanes])
    return c.finish()


def build_values(c):
    """every row of store_colours(), 64 to a wave over four pixels; the first two pixels' keys share a slot"""
    pool = special_colours()
    n = (len(pool) + 63) // 64
    rows = np.concatenate([pool, pool[:n * 64 - len(pool)]])
    for w in range(n):
        lanes = c.rng.permutation(64)
        c.wave([(21, 0, lanes[:20]), (21 + 64, 1, lanes[20:34]), (30, 2, lanes[34:50]), (31, 3, lanes[50:60])], colours=rows[64 * w:64 * w + 64])
    return c.finish()


def build_wraps(c):
    lanes = np.arange(64)
    up, down = np.full((64, 3), BIG, F32), np.full((64, 3), -BIG, F32)
    c.wave([(1, 0, lanes)], colours=up)                                                   # 64 lanes that each add INT32_MAX
    c.wave([(1, 0, lanes[:40]), (1 + 64, 1, lanes[40:])], colours=up)
    c.wave([(2, 0, lanes)], colours=down)
    # INT32_MIN and INT32_MAX mixed.  Lanes 0 .. 7, a pixel of their own: six up, two down -- out of int32; the rest of the wave as the seed has it
    mixed = np.where((c.rng.random((64, 1)) < 0.5), up, down).astype(F32)
    mixed[:6], mixed[6:8] = up[:6], down[:2]
    c.wave([(3, 0, lanes[:8]), (4, 1, lanes[8:])], colours=mixed)
    # even lanes one pixel, odd lanes another on the same slot: of lanes 0 .. 15 twelve up and four down, the rest of either pixel up and down in
    # equal numbers (each pair adds -1)
    halves = np.where((lanes // 2 % 2 == 0)[:, None], up, down).astype(F32)
    halves[:12], halves[12:16] = up[:12], down[:4]
    c.wave([(3, 0, lanes[lanes % 2 == 0]), (3 + 64, 1, lanes[lanes % 2 == 1])], colours=halves)
    return c.finish()


def build_wrap_from_acc(c):
    """the accumulator starts at INT32_MAX (INT32_MIN in the odd rows' pixels, whose lanes add negative colours): the first add wraps it"""
    lanes = np.arange(64)
    ones = np.full((64, 3), 1.0, F32)
    c.wave([(1, 0, [17])], colours=ones)
    c.wave([(1, 0, lanes), ], colours=c.rng.uniform(0.5, 4, (64, 3)).astype(F32))
    c.wave([(2, 0, lanes[:32]), (2 + 64, 2, lanes[32:])], colours=c.rng.uniform(0.5, 4, (64, 3)).astype(F32))
    c.wave([(5, 1, lanes[lanes % 2 == 0]), (6, 3, [1, 63])], colours=-ones)

    def acc(case):
        a = np.full((case.W, H, 3), INT32_MAX, I64)
        a[:, 1::2] = INT32_MIN
        return a.astype(I32)
    return c.finish(acc)


def build_stale_lds(c):
    lanes = np.arange(64)
    patterns = [
        [(5, 0, lanes)],
        [(5, 0, lanes[:10]), (9, 1, lanes[30:33])],
        [(5, 0, lanes[:32]), (5 + 64, 1, lanes[32:])],
        [(5, 0, lanes[(lanes % 2 == 1) & (lanes != 5)]), (5 + 64, 1, lanes[(lanes % 2 == 0) & (lanes != 20)]), (20, 2, [5, 20])],
    ]

    def preset(key_of, lane_of):
        def rows_of(rows, key, m):
            rows = rows.copy()
            for r in ROW_SUMS:
                rows[r] = np.where(rows[r] == 0, 1, rows[r])
            rows[ROW_SUMS[0]] = INT32_MAX
            for s in range(64):
                mine = np.flatnonzero(m & ((key & 63) == s))
                rows[ROW_KEY, s] = key_of(s, key, mine)
                rows[ROW_LANE, s] = lane_of(s, mine)
            return rows
        return rows_of
    own_first = lambda s, key, mine: key[mine[0]] if len(mine) else s
    own_last = lambda s, key, mine: key[mine[-1]] if len(mine) else s
    collider = lambda s, key, mine: (int(key[mine[0]]) // KEYS_PER_WAVE * KEYS_PER_WAVE + s + 64 * 40) if len(mine) else s      # no wave uses 40 * 64 + s
    lane_first = lambda s, mine: mine[0] if len(mine) else s
    lane_last = lambda s, mine: mine[-1] if len(mine) else 63 - s
    lane_self = lambda s, mine: s
    for groups in patterns:
        for key_of, lane_of in ((own_first, lane_first), (own_last, lane_last), (collider, lane_first), (collider, lane_self), (own_first, lane_self)):
            c.wave(groups, lds=preset(key_of, lane_of))
    return c.finish()


def build_across_waves(c):
    lanes = np.arange(64)
    for w in range(64):
        c.wave([(11, 2, lanes[lanes % 2 == w % 2]), (12, 7, lanes[lanes % 2 != w % 2])], colours=pool_colours(c.rng, special=0.1))
    return c.finish()


FUZZ_KEYS = ((5, 0), (5 + 64, 1), (17, 2), (17 + 128, 3), (40, 4), (22, 5))      # (local key, local pixel): two pairs share a slot


def build_fuzz(c):
    for _ in range(256):
        kind = c.rng.choice(5, p=(0.15, 0.15, 0.2, 0.25, 0.25))
        mask = np.ones(64, bool) if kind == 1 else np.zeros(64, bool) if kind == 0 else c.rng.random(64) < c.rng.uniform(0.05, 0.95)
        pool = (0, 2, 4, 5) if kind == 2 else range(6)               # kind 2: keys that do not collide
        pick = c.rng.choice(list(pool), 64)
        if kind == 3:                                                  # a collision of groups of at least two lanes each
            four = c.rng.permutation(64)[:4]
            mask[four] = True
            pick[four] = (0, 0, 1, 1) if c.rng.random() < 0.5 else (3, 2, 2, 3)
        c.wave([(FUZZ_KEYS[k][0], FUZZ_KEYS[k][1], np.flatnonzero(mask & (pick == k))) for k in range(6) if (mask & (pick == k)).any()],
               colours=pool_colours(c.rng))
    return c.finish()


# name -> (builder, property, Case arguments); the order is the seed's
CLASSES = {
    "one_pixel": (build_one_pixel, prop_one_pixel, {}),
    "one_lane": (build_one_lane, prop_one_lane, {}),
    "no_lane": (build_no_lane, prop_no_lane, {}),
    "order0_like": (build_order0_like, prop_order0_like, {"band": 13}),
    "split_pixels": (build_split_pixels, prop_split_pixels, {}),
    "collisions": (build_collisions, prop_collisions, {"band": 13}),
    "large_keys": (build_large_keys, prop_large_keys, {"keys_down": True}),
    "slot_vs_lane": (build_slot_vs_lane, prop_slot_vs_lane, {"band": 13}),
    "values_spp1": (build_values, prop_values, {"spp": 1}),
    "values_spp3": (build_values, prop_values, {"spp": 3}),
    "wraps": (build_wraps, prop_wraps, {}),
    "wrap_from_acc": (build_wrap_from_acc, prop_wraps, {}),
    "stale_lds": (build_stale_lds, prop_stale, {}),
    "across_waves": (build_across_waves, prop_across_waves, {"shared": True}),
    "fuzz": (build_fuzz, prop_fuzz, {}),
}
_cases = {}


def case(name):
    """the case of a class: built once, read-only"""
    if name not in _cases:
        build, _, kw = CLASSES[name]
        _cases[name] = build(Case(name, np.random.default_rng([SEED, list(CLASSES).index(name)]), **kw))
    return _cases[name]


def check_property(name, ints):
    CLASSES[name][1](case(name), ints)
