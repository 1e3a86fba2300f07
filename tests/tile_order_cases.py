"""Tile-cost planes for the tile-order feedback kernels, seeded, and the table of cases shared by tests/test_tile_order_host.py (no GPU: proves on
the reference of tests/tile_order_checks.py alone that every case reaches the edge it is named for) and tests/test_gpu_tile_order.py (the same
cases through dr_kat_tile_feedback).

The kernels' contract, kept by every case: 1 <= ntiles, regions 1 or 8, 8 regions only from 512 tiles on (regions of at least 64 tiles),
split_limit >= 0, and sum(tile costs) * heavy_factor < 2^64 -- tile_order_kernel forms that product in 64 bits and does not check it.

Tile counts: the smallest at which each path of tile_order_kernel exists.  Its 16 waves own consecutive ranges of `per` tiles, per = ceil(ntiles /
16) rounded up to 64, and walk them in groups of 64, eight groups per round: up to 1024 tiles a range is one group, 1025 is the first count with
two, 8320 (a 1024 x 520 frame, per = 576) the first in the table with a second round, 32400 is 1920 x 1080 (the benchmark: eight regions of 4050
tiles, ranges of 2048, region bounds in the middle of a group)."""
import numpy as np

import tile_order_checks as tc

TILE_COUNTS = (1, 63, 64, 65, 511, 512, 513, 575, 960, 1000, 1023, 1024, 1025, 8191, 8192, 8320, 32400)
HEAVY_FACTORS = (-1, 0, 1, 3, 1000)
SPLIT_STEPS = (0, 16, 400, 4080)
SPLIT_LIMITS = (0, 7, 64, 100000)          # 7 // 8 regions = 0
SPLITS = tuple((s, l) for s in SPLIT_STEPS for l in SPLIT_LIMITS)
U32_MAX = 2 ** 32 - 1
MAX_LANES = (0, 31, 32, 63)                # where a tile's maximum sits in its 64 pixel costs: both ends of both halves of the wave
WAVES = 16


def combos():
    """(ntiles, regions): one region everywhere, eight from 512 tiles on"""
    return [(n, r) for n in TILE_COUNTS for r in (1, 8) if r == 1 or n >= 64 * tc.MAX_REGIONS]


def wave_ranges(ntiles):
    """[w0, w1) of the 16 waves of tile_order_kernel (what the planes `range_ends` and the predicate `carry` are laid out against)"""
    per = (-(-ntiles // WAVES) + 63) // 64 * 64
    return [(min(w * per, ntiles), min(w * per + per, ntiles)) for w in range(WAVES)]


def _rng(ntiles, salt):
    return np.random.default_rng([ntiles, salt])


# ---- planes of tile costs: f(ntiles, regions) -> uint32[ntiles]
def zero(n, regions):
    return np.zeros(n, dtype=np.uint32)


def equal(n, regions):
    return np.full(n, 1234, dtype=np.uint32)


def random(n, regions):
    """uniform below 6000: 375 classes' worth folded into classes 0 .. 374 -> saturating only above 4080"""
    return _rng(n, 1).integers(0, 6000, size=n).astype(np.uint32)


def alternating(n, regions):
    """5000, 3, 5000, 3, ...: every ballot of 64 holds heavy and light tiles (heavy_factor 1: the mean is about 2500)"""
    c = np.full(n, 3, dtype=np.uint32)
    c[0::2] = 5000
    return c


def saturating(n, regions):
    """half of the tiles (seeded choice) 0, the others uniform up to 70000: classes far beyond 255"""
    rng = _rng(n, 2)
    c = rng.integers(1, 70001, size=n).astype(np.uint32)
    c[rng.random(n) < 0.5] = 0
    return c


def thirds(n, regions):
    """16, 32, 48 in turn; with ntiles divisible by 3 the mean is exactly 32: a third of the tiles sit on the threshold of heavy_factor 1"""
    assert n % 3 == 0
    return np.array([16, 32, 48], dtype=np.uint32)[np.arange(n) % 3]


def region_blocks(n, regions):
    """regions 2 and 5 of eight all heavy (4000 .. 6000: several classes), every other region below 100 (heavy_factor 1: the mean is above 1000)"""
    assert regions == 8
    rb = tc.region_bounds(n, regions)
    rng = _rng(n, 3)
    c = rng.integers(0, 100, size=n).astype(np.uint32)
    for r in (2, 5):
        c[rb[r]:rb[r + 1]] = rng.integers(4000, 6001, size=rb[r + 1] - rb[r]).astype(np.uint32)
    return c


def range_ends(n, regions):
    """5000 at the first and the last tile of each wave's range, 3 elsewhere"""
    c = np.full(n, 3, dtype=np.uint32)
    for w0, w1 in wave_ranges(n):
        if w1 > w0:
            c[w0] = 5000
            c[w1 - 1] = 5000
    return c


def huge(n, regions):
    """uniform below 2^32 with the two ends of the range present: the total needs 64 bits"""
    c = _rng(n, 4).integers(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    c[n // 2] = U32_MAX
    c[n // 3] = 0
    return c


PLANES = {f.__name__: f for f in (zero, equal, random, alternating, saturating, thirds, region_blocks, range_ends, huge)}


def pixels(cost):
    """A flat plane of len(cost) * 64 pixel costs whose tile maxima are `cost`: the maximum at lane 0, 31, 32 or 63 (by tile number), the other
    lanes uniform in [0, cost]"""
    cost = np.asarray(cost, dtype=np.uint32)
    n = len(cost)
    rng = np.random.default_rng([n, int(cost[0]), 5])
    p = (rng.integers(0, 2 ** 32, size=(n, 64), dtype=np.uint64) % (cost.astype(np.uint64)[:, None] + np.uint64(1))).astype(np.uint32)
    p[np.arange(n), np.array(MAX_LANES)[np.arange(n) % 4]] = cost
    return p.ravel()


# ---- the edges a case can be named for, decided on the reference alone
def carry(ref, cost):
    """Some wave's range holds light tiles of region r + 1 both in the 64-tile group that straddles rb[r + 1] and in a later group of the range:
    the wave's count of light tiles already placed in region r + 1 must travel with it when r + 1 becomes its current region"""
    light = ~ref.heavy
    for w0, w1 in wave_ranges(ref.ntiles):
        for r in range(ref.regions - 1):
            b, e = ref.rb[r + 1], ref.rb[r + 2]
            if not (w0 < b < w1) or (b - w0) % 64 == 0:
                continue
            g1 = w0 + ((b - w0) // 64 + 1) * 64                 # end of the straddling group
            if light[b:min(g1, w1, e)].any() and g1 < min(w1, e) and light[g1:min(w1, e)].any():
                return True
    return False


def edges(ref, cost):
    cost = np.asarray(cost, dtype=np.uint32)
    per_region = [ref.heavy[ref.rb[r]:ref.rb[r + 1]] for r in range(ref.regions)]
    found = set()
    if ref.regions > 1 and carry(ref, cost):
        found.add("carry")
    if ref.threshold is not None and ref.threshold < 2 ** 32 and (cost == ref.threshold).any():      # (heavy_factor -1: tiles of cost 0)
        found.add("exact_threshold")
    if (ref.heavy & ((cost >> 4) > tc.CLASSES - 1)).any():
        found.add("saturated_class")
    if any(c > 0 for c in ref.counts):
        found.add("split")
    if getattr(ref, "split_over_limit", False):
        found.add("split_capped")
    if any(not h.any() for h in per_region):
        found.add("region_without_heavy")
    if ref.heavy.all():
        found.add("every_tile_heavy")
    if ref.heavy.any() and not ref.heavy.all():
        found.add("mixed")
    if len(set(ref.cls[ref.heavy].tolist())) > 1:
        found.add("several_classes")
    if tc.total_cost(cost) >= 2 ** 32:
        found.add("total_64_bits")
    return found


class Case:
    def __init__(self, ntiles, regions, plane, heavy_factor, split, expect=()):
        self.ntiles, self.regions, self.plane, self.heavy_factor = ntiles, regions, plane, heavy_factor
        self.split_steps, self.split_limit = split
        self.expect = frozenset(expect)            # the edges the host test asserts this case reaches
        self.name = "%s-%dt-%dr-hf%d-s%d-l%d" % (plane, ntiles, regions, heavy_factor, self.split_steps, self.split_limit)

    def cost(self):
        return PLANES[self.plane](self.ntiles, self.regions)

    def reference(self, cost=None):
        cost = self.cost() if cost is None else cost
        ref = tc.Reference(cost, self.regions, self.heavy_factor, self.split_steps, self.split_limit)
        ref.split_over_limit = any(n > self.split_limit // self.regions for n in ref.long_ones)      # (the predicate "split capped")
        return ref


def _table():
    cases = []
    k = 0                                            # walks the 16 split pairs and the heavy factors so that all of them meet every plane

    def add(n, r, plane, hf, expect=(), split=None):
        nonlocal k
        cases.append(Case(n, r, plane, hf, SPLITS[k % len(SPLITS)] if split is None else split, expect))
        k += split is None

    for i, (n, r) in enumerate(combos()):
        multi = n >= 64                              # enough tiles for both kinds and several classes
        deep = r == 8 and n > 1024                   # more than one group per wave and region bounds inside the ranges
        add(n, r, "random", 1, (("mixed", "several_classes") if multi else ()) + carries_of(n, r, 1))
        add(n, r, "alternating", HEAVY_FACTORS[i % 5])
        add(n, r, "saturating", (1, -1)[i % 2], ("saturated_class", "split") if multi else (), split=(4080, (100000, 64)[i % 2]))
        if multi and (deep or i % 2):
            add(n, r, "range_ends", 1, ("mixed",) + carries_of(n, r, 1))
        else:
            add(n, r, ("zero", "equal")[(i // 2) % 2], HEAVY_FACTORS[(i // 4) % 5])
    # every other heavy factor on one plane at the shapes with two groups per wave and a second round
    for n, r in ((1025, 8), (8320, 8), (32400, 8)):
        for hf in (-1, 0, 3, 1000):
            add(n, r, "random", hf, carries_of(n, r, hf))
    add(32400, 1, "random", 3)
    add(32400, 1, "random", -1)
    # strictness of the threshold: a third of the tiles cost exactly the mean; all-equal planes are on it with every tile
    for n, r in ((63, 1), (513, 1), (513, 8), (960, 8), (1023, 8), (32400, 1), (32400, 8)):
        add(n, r, "thirds", 1, ("exact_threshold", "mixed"), split=(16, 100000))
    for n, r in ((1, 1), (64, 1), (1025, 8)):
        add(n, r, "equal", 1, ("exact_threshold", "region_without_heavy"))
    for n, r in ((1, 1), (65, 1), (1025, 8), (8320, 8)):
        add(n, r, "equal", -1, ("every_tile_heavy",), split=(400, 64))
    # one region all heavy, its neighbours all light
    for n in (512, 513, 1025, 8320, 32400):
        add(n, 8, "region_blocks", 1, ("region_without_heavy", "several_classes", "split", "split_capped"), split=(400, 64))
    add(1000, 8, "region_blocks", 1, ("region_without_heavy",), split=(400, 7))          # 7 // 8 = 0: nothing split
    # costs up to 2^32 - 1: the sum needs 64 bits (heavy_factor <= 1 keeps the product below 2^64)
    for r in (1, 8):
        for hf in (-1, 0, 1):
            add(1025, r, "huge", hf, ("total_64_bits",) + (("saturated_class", "mixed") if hf else ()), split=(4080, 100000))
    # the split limit below the count at one region too
    add(960, 1, "alternating", 1, ("split", "split_capped"), split=(16, 64))
    add(8192, 1, "saturating", -1, ("split", "split_capped", "saturated_class"), split=(4080, 7))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cases


def carries_of(n, r, hf):
    """(8191 and 8192 tiles have their region bounds on group bounds: nothing straddles; heavy_factor -1 on a plane without zeros leaves no light tile)"""
    return ("carry",) if r == 8 and n in (1025, 8320, 32400) and hf != -1 else ()


CASES = _table()
BY_NAME = {c.name: c for c in CASES}

# pixel planes for tile_cost_kernel alone (four tiles per block): tile counts that are no multiple of 4, costs over the whole uint32 range
TILE_COST_COUNTS = (1, 2, 3, 5, 63, 65, 1023, 1025, 8191)
