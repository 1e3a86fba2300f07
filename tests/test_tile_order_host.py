"""The cases of tests/test_gpu_tile_order.py are fair -- checked without a GPU, on the reference of tests/tile_order_checks.py alone.  For the
table of tests/tile_order_cases.py this file asserts the conditions that make the GPU comparison mean something:

  * the reference is what the contract says: worked by hand on small planes, and equal to a second restatement in plain Python integers and
    sorted() on every case of up to 1025 tiles;
  * every case reaches the edge it is named for (conditions, not measurements): a wave range that carries its light-tile count across a region
    bound, tiles exactly on the threshold, classes beyond 255, a split count above its limit, a region without heavy tiles, every tile heavy,
    a total that needs 64 bits -- and the carry is reached at each of 1025, 8320 and 32400 tiles with eight regions;
  * every case keeps the kernels' contract (sum * heavy_factor < 2^64, regions of at least 64 tiles);
  * the comparison function reports a duplicate, a hole, a tile of another region, a wrong class, light tiles out of order, a wrong start and a
    wrong count, and accepts any order inside a class;
  * four value mutants of the contract, restated here (cost >= threshold, classes ascending, region bounds rounded down, the split test on the
    saturated class with >), are each reported for some case: a device kernel with one of these mistakes cannot pass the table."""
import numpy as np
import pytest

import tile_order_cases as cs
import tile_order_checks as tc


def restated(cost, regions, heavy_factor, split_steps, split_limit, mutant=None):
    """(order, region_start[17]) from Python integers alone; mutant: None or one of 'ge', 'ascending', 'floor', 'split_saturated'"""
    cost = [int(c) for c in cost]
    n = len(cost)
    rb = [(r * n) // regions if mutant == "floor" else -((-r * n) // regions) for r in range(regions + 1)]
    thr = None if heavy_factor == 0 else (0 if heavy_factor < 0 else sum(cost) * heavy_factor // n)
    if mutant == "ge":
        heavy = [thr is not None and c >= thr for c in cost]
    else:
        heavy = [thr is not None and c > thr for c in cost]
    cls = [min(c >> 4, 255) for c in cost]
    order, words = [], [-1] * tc.WORDS
    for r in range(regions):
        tiles = range(rb[r], rb[r + 1])
        hv = sorted((t for t in tiles if heavy[t]), key=lambda t: ((cls[t] if mutant == "ascending" else -cls[t]), t))
        order += hv + [t for t in tiles if not heavy[t]]
        if mutant == "split_saturated":
            long_ones = sum(1 for t in hv if cls[t] > (split_steps >> 4))
        else:
            long_ones = sum(1 for t in hv if (cost[t] >> 4) >= (split_steps >> 4))
        words[tc.MAX_REGIONS + 1 + r] = min(long_ones, split_limit // regions) if split_steps > 0 else 0
        words[r] = rb[r]
    words[regions] = n
    return np.array(order, dtype=np.int32), np.array(words, dtype=np.int32)


def words_of(ref):
    w = np.full(tc.WORDS, -1, dtype=np.int32)
    w[:ref.regions + 1] = ref.rb
    w[tc.MAX_REGIONS + 1:tc.MAX_REGIONS + 1 + ref.regions] = ref.counts
    return w


def test_reference_by_hand():
    # eight tiles, one region, heavy_factor 1: sum 800, threshold 100 -> heavy are 101 (class 6), 340 (class 21), 199 (class 12); 100 is not
    cost = np.array([100, 101, 20, 340, 0, 199, 30, 10], dtype=np.uint32)
    ref = tc.Reference(cost, 1, 1, 0, 0)
    assert ref.threshold == 100 and ref.rb == [0, 8]
    assert ref.order.tolist() == [3, 5, 1, 0, 2, 4, 6, 7] and ref.label.tolist() == [21, 12, 6, -1, -1, -1, -1, -1] and ref.counts == [0]
    # split: cost >> 4 >= 192 >> 4 = 12 holds for 340 and 199; the limit lets one through
    assert tc.Reference(cost, 1, 1, 192, 100).counts == [2] and tc.Reference(cost, 1, 1, 192, 1).counts == [1] and tc.Reference(cost, 1, 1, 192, 0).counts == [0]
    # heavy_factor -1: every tile above 0 by class, ties by tile number; 0: the natural order
    assert tc.Reference(cost, 1, -1, 0, 0).order.tolist() == [3, 5, 0, 1, 2, 6, 7, 4]
    assert tc.Reference(cost, 1, 0, 400, 64).order.tolist() == list(range(8)) and tc.Reference(cost, 1, 0, 400, 64).counts == [0]
    # classes saturate: 4080 and 70000 share class 255, 4079 is class 254
    sat = tc.Reference(np.array([4079, 70000, 4080, 0], dtype=np.uint32), 1, -1, 4080, 8)
    assert sat.order.tolist() == [1, 2, 0, 3] and sat.label.tolist() == [255, 255, 254, -1] and sat.counts == [2]
    # region bounds round up: 513 tiles in 8 regions
    assert tc.region_bounds(513, 8) == [0, 65, 129, 193, 257, 321, 385, 449, 513] and tc.region_bounds(32400, 8)[1] == 4050
    assert tc.total_cost(np.full(3, 2 ** 32 - 1, dtype=np.uint32)) == 3 * (2 ** 32 - 1)
    assert tc.threshold(np.full(1025, 2 ** 32 - 1, dtype=np.uint32), 1) == 2 ** 32 - 1 and tc.threshold(cost, 0) is None and tc.threshold(cost, -1) == 0
    pix = np.zeros(2 * 64, dtype=np.uint32)
    pix[63], pix[64], pix[70] = 9, 4, 5
    assert tc.tile_cost(pix, 2).tolist() == [9, 5]


def test_table_covers_what_it_should():
    assert 140 <= len(cs.CASES) <= 165 and len(cs.BY_NAME) == len(cs.CASES)
    assert {(c.ntiles, c.regions) for c in cs.CASES} == set(cs.combos()) and len(cs.combos()) == 29
    assert all(c.regions == 1 or c.ntiles >= 512 for c in cs.CASES)
    assert {c.heavy_factor for c in cs.CASES} == set(cs.HEAVY_FACTORS)
    assert {(c.split_steps, c.split_limit) for c in cs.CASES} == set(cs.SPLITS)
    assert {c.plane for c in cs.CASES} == set(cs.PLANES)
    for n, r in ((1025, 8), (8320, 8), (32400, 8)):                     # every heavy factor where a wave has several groups
        assert {c.heavy_factor for c in cs.CASES if (c.ntiles, c.regions) == (n, r)} == set(cs.HEAVY_FACTORS)
    assert {c.heavy_factor for c in cs.CASES if c.plane == "huge"} == {-1, 0, 1} and {c.ntiles for c in cs.CASES if c.plane == "huge"} == {1025}
    assert all(n % 4 for n in cs.TILE_COST_COUNTS)
    # the kernel's ranges as the planes and the carry predicate see them
    assert cs.wave_ranges(1024)[15] == (960, 1024) and cs.wave_ranges(1025)[:2] == [(0, 128), (128, 256)] and cs.wave_ranges(1025)[9] == (1025, 1025)
    assert cs.wave_ranges(8320)[1] == (576, 1152) and cs.wave_ranges(32400)[15] == (30720, 32400)


def test_generators():
    for name, f in cs.PLANES.items():
        for n, r in ((960, 8), (1023, 1)):
            if name == "region_blocks" and r != 8:
                continue
            a = f(n, r)
            assert a.dtype == np.uint32 and a.shape == (n,) and np.array_equal(a, f(n, r)), name
    assert cs.huge(1025, 1).max() == cs.U32_MAX and cs.huge(1025, 1).min() == 0 and cs.saturating(1025, 1).max() > 4096 * 16
    for n in cs.TILE_COST_COUNTS:
        cost = cs.huge(n, 1) if n > 3 else np.array([7, 0, cs.U32_MAX][:n], dtype=np.uint32)
        pix = cs.pixels(cost)
        assert pix.dtype == np.uint32 and pix.shape == (n * 64,) and np.array_equal(tc.tile_cost(pix, n), cost)
        if n >= 63:
            t = np.flatnonzero(cost > 64)                               # (a small maximum may tie with another lane)
            first = pix.reshape(n, 64)[t].argmax(axis=1)
            assert set(first.tolist()) == set(cs.MAX_LANES) and np.array_equal(first, np.array(cs.MAX_LANES)[t % 4])


@pytest.fixture(scope="module")
def worked():
    """name -> (case, cost, reference, edges), computed once"""
    out = {}
    for c in cs.CASES:
        cost = c.cost()
        ref = c.reference(cost)
        out[c.name] = (c, cost, ref, cs.edges(ref, cost))
    return out


def pick(worked, plane, ntiles, regions, heavy_factor):
    return next(v for v in worked.values() if (v[0].plane, v[0].ntiles, v[0].regions, v[0].heavy_factor) == (plane, ntiles, regions, heavy_factor))


def test_every_case_reaches_its_edge_and_keeps_the_contract(worked):
    reached = {}
    for name, (c, cost, ref, found) in worked.items():
        assert c.expect <= found, (name, sorted(c.expect - found))
        assert tc.total_cost(cost) * max(c.heavy_factor, 0) < 2 ** 64, name
        assert c.split_limit >= 0 and c.ntiles >= 1 and min(b - a for a, b in zip(ref.rb, ref.rb[1:])) >= (64 if c.regions == 8 else 1), name
        assert sorted(ref.order.tolist()) == list(range(c.ntiles)), name
        assert tc.first_difference(ref, ref.order, words_of(ref)) is None, name
        for e in found:
            reached.setdefault(e, set()).add((c.ntiles, c.regions))
    assert set(reached) == {"carry", "exact_threshold", "saturated_class", "split", "split_capped", "region_without_heavy", "every_tile_heavy", "mixed",
                            "several_classes", "total_64_bits"}
    assert reached["carry"] == {(1025, 8), (8320, 8), (32400, 8)}          # up to 1024 tiles, and with bounds on group bounds, nothing is carried
    assert {(513, 8), (960, 8), (1023, 8), (32400, 8), (63, 1)} <= reached["exact_threshold"]
    assert {(1, 1), (8320, 8)} <= reached["every_tile_heavy"] and {(8, ), (1, )} == {(r, ) for _, r in reached["split_capped"]}
    # split_limit 7 with eight regions lets nothing through although tiles qualify
    c, cost, ref, found = pick(worked, "region_blocks", 1000, 8, 1)
    assert ref.counts == [0] * 8 and "split_capped" in found


def test_reference_equals_the_plain_python_restatement(worked):
    for name, (c, cost, ref, _) in worked.items():
        if c.ntiles > 1025:
            continue
        order, words = restated(cost, c.regions, c.heavy_factor, c.split_steps, c.split_limit)
        assert np.array_equal(order, ref.order) and np.array_equal(words, words_of(ref)), name


def test_comparison_reports_each_kind_of_difference(worked):
    c, cost, ref, _ = pick(worked, "random", 1025, 8, 1)
    good, words = ref.order.copy(), words_of(ref)
    assert tc.first_difference(ref, good, words) is None
    light = np.flatnonzero(ref.label < 0)
    heavy = np.flatnonzero(ref.label >= 0)
    run = next(p for p in heavy[:-1] if ref.label[p] == ref.label[p + 1] and p + 1 not in ref.rb)

    def changed(f, w=None):
        o, ww = good.copy(), words.copy()
        f(o, ww)
        return tc.first_difference(ref, o, ww)

    def swap(o, a, b):
        o[a], o[b] = o[b], o[a]

    assert changed(lambda o, w: swap(o, run, run + 1)) is None                        # inside a class any order will do
    assert "no tile" in changed(lambda o, w: o.__setitem__(5, -1))
    assert "no tile" in changed(lambda o, w: o.__setitem__(5, c.ntiles))
    assert "appears 2 times" in changed(lambda o, w: o.__setitem__(light[3], o[light[4]])) or "appears 0 times" in changed(lambda o, w: o.__setitem__(light[3], o[light[4]]))
    assert "natural order" in changed(lambda o, w: swap(o, light[3], light[4]))
    assert "expected a tile that is" in changed(lambda o, w: swap(o, heavy[0], light[0]))
    p = next(p for p in heavy[:-1] if ref.label[p] != ref.label[p + 1] and p + 1 not in ref.rb and ref.label[p + 1] >= 0)
    assert "heavy of class" in changed(lambda o, w: swap(o, p, p + 1))
    assert "another region" in changed(lambda o, w: swap(o, light[0], light[-1]))
    assert "region_start[3]" in changed(lambda o, w: w.__setitem__(3, w[3] - 1))
    assert "region_start[8]" in changed(lambda o, w: w.__setitem__(8, -1))
    c2, cost2, ref2, _ = pick(worked, "region_blocks", 1025, 8, 1)
    w2 = words_of(ref2)
    w2[tc.MAX_REGIONS + 1 + 2] -= 1
    assert "split count of region 2" in tc.first_difference(ref2, ref2.order, w2)
    w2 = words_of(ref2)
    w2[12:] = 77                                                                      # words nobody reads are not compared ...
    c1, cost1, ref1, _ = pick(worked, "random", 1025, 1, 1)
    w1 = words_of(ref1)
    w1[2:9] = 77
    w1[10:] = 77                                                                      # ... (one region: words 2 .. 8 and 10 .. 16)
    assert tc.first_difference(ref1, ref1.order, w1) is None


MUTANTS = ("ge", "ascending", "floor", "split_saturated")


@pytest.mark.parametrize("mutant", MUTANTS)
def test_value_mutants_of_the_contract_are_reported(worked, mutant):
    """Each mutant restated in plain Python differs from the reference for some case, and -- for the two the issue predicts -- only where the named
    edge is reached"""
    caught = []
    for name, (c, cost, ref, found) in worked.items():
        if c.ntiles > 1025:
            continue
        order, words = restated(cost, c.regions, c.heavy_factor, c.split_steps, c.split_limit, mutant)
        if tc.first_difference(ref, order, words) is not None:
            caught.append(name)
            if mutant == "ge":
                assert "exact_threshold" in found, name
            if mutant == "floor":
                assert c.regions == 8 and c.ntiles % 8, name
    assert len(caught) >= 3, caught
