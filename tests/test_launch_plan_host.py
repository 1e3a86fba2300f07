"""Which build of the persistent kernel a launch runs (dogeray_amd/csrc/launch_plan.hpp plan_persistent, through tools/host_kernel.cpp), checked
without a GPU against a plain-Python restatement of the four launcher functions the plan replaced -- launch_persistent_kernel, launch_wide_lean6,
launch_persistent_occ<OCC> and launch_persistent<...> of kernels_render.hip -- and of the two launch-size rules of context_render.cpp (the queue
count of make_params, split_limit of enqueue_frame), written from their text function by function, oddities included:

  * the plan equals the restatement field for field on the whole grid (traversal, occupancy, schedule, counting, CUs, tiles per wave, coop_steps, wave
    log, per-frame stores, and work on both sides of every threshold);
  * every planned build is instantiated (DR_PERSISTENT_BUILDS), every instantiated build is planned somewhere, and the list has no duplicates;
  * the queue count and split_limit equal their restatements;
  * five mutants of the restatement -- mistakes a change to the plan could make -- each differ from the plan, first at the grid point named here."""
import itertools
import os
import sys
from collections import namedtuple

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

THREADED, WIDE = 0, 2                    # DR_TRAVERSAL_THREADED, DR_TRAVERSAL_WIDE
WAVE_LOG_WAVES = 16384
MAX_REGIONS = 8
Cfg = namedtuple("Cfg", "traversal occupancy schedule num_cus coop_tiles_per_wave count")
Launch = namedtuple("Launch", "build blocks log_waves wave_log_cleared")      # build: the eight template arguments, as ints
MUTANTS = ("unclamped", "le", "coop_first", "six_schedule_1", "threaded_log_zero")


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


# ---------------------------------------------------------------- the parent's launchers, restated
def launch_persistent(cfg, OCC, TRAV_MIN, PARK_MIN, P_UNROLL, COOP_PARK, COOP_UNROLL, work, coop_steps, wave_log, mutant):
    blocks = cfg.num_cus * OCC
    if blocks * 4 > work:
        blocks = (work + 3) // 4
    cleared = False
    if wave_log and blocks * 4 > WAVE_LOG_WAVES:
        wave_log, cleared = False, True
    log_waves = blocks * 4 if wave_log else 0
    if cfg.traversal == WIDE:
        waves = cfg.num_cus * OCC * 4 if mutant == "unclamped" else blocks * 4
        limit = cfg.coop_tiles_per_wave * waves
        coop = coop_steps > 0 and (work <= limit if mutant == "le" else work < limit)
        if not coop:
            log_waves = 0
        if mutant == "coop_first" and coop:
            return Launch((0, OCC, TRAV_MIN, COOP_PARK, COOP_UNROLL, 1, 1, 0), blocks, log_waves, cleared)
        if cfg.count:
            return Launch((1, OCC, TRAV_MIN, PARK_MIN, P_UNROLL, 1, 0, 0), blocks, log_waves, cleared)
        if coop:
            return Launch((0, OCC, TRAV_MIN, COOP_PARK, COOP_UNROLL, 1, 1, 0), blocks, log_waves, cleared)
        return Launch((0, OCC, TRAV_MIN, PARK_MIN, P_UNROLL, 1, 0, 0), blocks, log_waves, cleared)
    if mutant == "threaded_log_zero":
        log_waves = 0
    # (the threaded instantiations leave COOP at the template's default, true)
    return Launch((1 if cfg.count else 0, OCC, TRAV_MIN, PARK_MIN, P_UNROLL, 0, 1, 0), blocks, log_waves, cleared)


def launch_persistent_occ(cfg, OCC, work, coop_steps, wave_log, mutant):
    if cfg.schedule == 0:
        return launch_persistent(cfg, OCC, 32, 20, 2, 12, 4, work, coop_steps, wave_log, mutant)
    if cfg.schedule == 1:
        return launch_persistent(cfg, OCC, 32, 8, 1, 8, 1, work, coop_steps, wave_log, mutant)
    return launch_persistent(cfg, OCC, 48, 0, 1, 0, 1, work, coop_steps, wave_log, mutant)


def launch_wide_lean6(cfg, work, coop_steps, out_frame_stride, mutant):
    """None: not launched"""
    if cfg.traversal != WIDE or cfg.count or (cfg.schedule != 0 and not (mutant == "six_schedule_1" and cfg.schedule == 1)):
        return None
    limit = cfg.coop_tiles_per_wave * cfg.num_cus * 5 * 4
    if coop_steps > 0 and (work <= limit if mutant == "le" else work < limit):
        return None
    blocks = cfg.num_cus * 6
    if blocks * 4 > work:
        blocks = (work + 3) // 4
    return Launch((0, 6, 32, 20, 2, 1, 0, 1 if out_frame_stride else 0), blocks, 0, True)


def can_store_per_frame(cfg):
    return cfg.traversal == WIDE and not cfg.count and cfg.schedule == 0 and cfg.occupancy >= 6


def launch_persistent_kernel(cfg, work, coop_steps, out_frame_stride, wave_log, mutant=None):
    if out_frame_stride and can_store_per_frame(cfg):
        six = launch_wide_lean6(cfg, work, coop_steps, out_frame_stride, mutant)
        if six:
            return six
        blocks = cfg.num_cus * 5
        if blocks * 4 > work:
            blocks = (work + 3) // 4
        cleared = False
        if wave_log and blocks * 4 > WAVE_LOG_WAVES:
            wave_log, cleared = False, True
        return Launch((0, 5, 32, 12, 4, 1, 1, 1), blocks, blocks * 4 if wave_log else 0, cleared)
    if cfg.occupancy >= 6:
        six = launch_wide_lean6(cfg, work, coop_steps, out_frame_stride, mutant)
        if six:
            return six
    if cfg.occupancy >= 5:
        return launch_persistent_occ(cfg, 5, work, coop_steps, wave_log, mutant)
    return launch_persistent_occ(cfg, 4, work, coop_steps, wave_log, mutant)


# ---------------------------------------------------------------- the parent's launch-size rules, restated
def regions_of(tiles, batch_hint, xcd_regions, short_one_queue, tiles_per_wave, num_cus):
    regions = MAX_REGIONS if xcd_regions else 1
    if tiles < 64 * MAX_REGIONS:
        regions = 1
    if short_one_queue and tiles * batch_hint < tiles_per_wave * num_cus * 20:
        regions = 1
    return regions


def split_limit_of(num_cus, occupancy, split_parts, split_waves):
    return num_cus * (5 if occupancy >= 5 else 4) * 4 * split_waves // (100 * split_parts) if split_parts > 1 else 0


# ---------------------------------------------------------------- the grid
NUM_CUS = (1, 8, 256, 1024)
TILES_PER_WAVE = (0, 1, 32, 100000)


def works(num_cus, tpw):
    w = {1, 3, 4, 5, 10 ** 7}
    thresholds = [WAVE_LOG_WAVES, tpw * num_cus * 20]
    for occ in (4, 5, 6):
        thresholds += [num_cus * occ * 4, tpw * num_cus * occ * 4]      # the grid's waves; the short-launch bound of a grid that is not clamped
    for t in thresholds:
        w |= {t - 1, t, t + 1}
    return sorted(v for v in w if v >= 1)


def grid():
    """(cfg, work, coop_steps, per_frame, wave_log) in a fixed order"""
    for traversal, occupancy, schedule, count, num_cus, tpw in itertools.product((THREADED, WIDE), (4, 5, 6), (0, 1, 2), (0, 1), NUM_CUS, TILES_PER_WAVE):
        cfg = Cfg(traversal, occupancy, schedule, num_cus, tpw, count)
        for coop_steps, wave_log, per_frame in itertools.product((0, 2), (0, 1), (0, 1)):
            if per_frame and not can_store_per_frame(cfg):      # (a caller sets a frame stride only where the predicate allows it)
                continue
            for work in works(num_cus, tpw):
                yield cfg, work, coop_steps, per_frame, wave_log


def as_plan(launch):
    return tuple(launch.build) + (launch.blocks, launch.log_waves, int(launch.wave_log_cleared))


@pytest.fixture(scope="module")
def planned(hk):
    """[(grid point, the plan)] over the whole grid, computed once"""
    return [(pt, hk.persistent_plan(pt[0]._asdict(), pt[1], pt[2], pt[3], pt[4])) for pt in grid()]


def test_the_restatement_by_hand():
    bench = Cfg(WIDE, 6, 0, 256, 32, 0)
    # 32 frames of 1920x1080 (32400 tiles each): long, the six-wave lean build on every CU; one frame: short, five waves, work sharing, and a log
    assert launch_persistent_kernel(bench, 32400 * 32, 2, 0, True) == Launch((0, 6, 32, 20, 2, 1, 0, 0), 1536, 0, True)
    assert launch_persistent_kernel(bench, 32400, 2, 0, True) == Launch((0, 5, 32, 12, 4, 1, 1, 0), 1280, 5120, False)
    assert launch_persistent_kernel(bench, 32400, 2, 0, False) == Launch((0, 5, 32, 12, 4, 1, 1, 0), 1280, 0, False)
    # a group of eight frames stored one by one: long enough at 320x192 on 8 CUs, short on 256
    assert launch_persistent_kernel(bench._replace(num_cus=8), 960 * 8, 2, 1, False).build == (0, 6, 32, 20, 2, 1, 0, 1)
    assert launch_persistent_kernel(bench, 960 * 8, 2, 1, False) == Launch((0, 5, 32, 12, 4, 1, 1, 1), 1280, 0, False)
    # 256 tiles: 64 workgroups wherever there are 16 CUs
    assert launch_persistent_kernel(bench, 256, 2, 0, True) == Launch((0, 5, 32, 12, 4, 1, 1, 0), 64, 256, False)
    assert launch_persistent_kernel(bench._replace(coop_tiles_per_wave=0), 256, 2, 0, True) == Launch((0, 6, 32, 20, 2, 1, 0, 0), 64, 0, True)
    # the oddities: the counting build of a short launch and the threaded builds report waves that never log; 1280 * 4 waves of 1024 CUs do not fit the log
    assert launch_persistent_kernel(bench._replace(count=1), 32400, 2, 0, True) == Launch((1, 5, 32, 20, 2, 1, 0, 0), 1280, 5120, False)
    assert launch_persistent_kernel(bench._replace(traversal=THREADED, schedule=2), 32400, 2, 0, True) == Launch((0, 5, 48, 0, 1, 0, 1, 0), 1280, 5120, False)
    assert launch_persistent_kernel(bench._replace(num_cus=1024, occupancy=5), 10 ** 7, 2, 0, True) == Launch((0, 5, 32, 20, 2, 1, 0, 0), 5120, 0, True)
    # ... and the two wave counts: with one tile per wave and work = four times a clamped grid, six waves are refused (unclamped: 4 < 20) and the
    # five-wave launch then finds itself long enough (clamped: 4 < 4 fails): the lean five-wave build
    assert launch_persistent_kernel(bench._replace(num_cus=1, coop_tiles_per_wave=1), 4, 2, 0, True) == Launch((0, 5, 32, 20, 2, 1, 0, 0), 1, 0, False)


def test_plan_equals_the_restatement_on_the_whole_grid(hk, planned):
    assert len(planned) > 40000
    for (cfg, work, coop_steps, per_frame, wave_log), plan in planned:
        want = as_plan(launch_persistent_kernel(cfg, work, coop_steps, per_frame, bool(wave_log)))
        assert plan == want, (cfg, work, coop_steps, per_frame, wave_log, dict(zip(hk.PLAN_FIELDS, zip(plan, want))))
    for traversal, occupancy, schedule, count in itertools.product((THREADED, WIDE), (4, 5, 6), (0, 1, 2), (0, 1)):
        cfg = Cfg(traversal, occupancy, schedule, 256, 32, count)
        assert hk.persistent_can_store_per_frame(cfg._asdict()) == can_store_per_frame(cfg), cfg


def test_planned_builds_are_the_instantiated_builds(hk, planned):
    builds = hk.persistent_builds()
    assert len(builds) == 33 and len(set(builds)) == 33
    used = {plan[:8] for _, plan in planned}
    assert used <= set(builds), sorted(used - set(builds))
    assert set(builds) <= used, sorted(set(builds) - used)          # no dead instantiation
    assert hk.BUILD_FIELDS == ("count", "occ", "trav_min", "park_min", "unroll", "wide", "coop", "perframe")
    for b in builds:
        count, occ, trav_min, park_min, unroll, wide, coop, perframe = b
        assert occ in (4, 5, 6) and (trav_min, park_min, unroll) in ((32, 20, 2), (32, 12, 4), (32, 8, 1), (48, 0, 1)), b
        assert (occ == 6) <= (b[:7] == (0, 6, 32, 20, 2, 1, 0)) and perframe <= (wide and not count), b


def test_queue_count_and_split_limit_equal_their_restatements(hk):
    seen = set()
    for tiles, hint, xcd, one, tpw, cus in itertools.product((1, 511, 512, 32400), (1, 8, 32), (0, 1), (0, 1), (0, 32, 500), NUM_CUS):
        got = hk.plan_regions(tiles, hint, xcd, one, tpw, cus)
        assert got == regions_of(tiles, hint, xcd, one, tpw, cus), (tiles, hint, xcd, one, tpw, cus)
        seen.add(got)
    assert seen == {1, MAX_REGIONS}
    assert hk.plan_regions(32400, 1, 1, 1, 32, 256) == 1 and hk.plan_regions(32400, 32, 1, 1, 32, 256) == 8 and hk.plan_regions(32400, 1, 1, 0, 32, 256) == 8
    assert hk.plan_regions(5120, 1, 1, 1, 1, 256) == 8 and hk.plan_regions(5119, 1, 1, 1, 1, 256) == 1          # tiles < tpw * num_cus * 20, strictly
    for cus, occupancy, parts, waves in itertools.product(NUM_CUS, (4, 5, 6), (1, 2, 4, 8), (1, 12, 1000)):
        assert hk.plan_split_limit(cus, occupancy, parts, waves) == split_limit_of(cus, occupancy, parts, waves), (cus, occupancy, parts, waves)
    assert hk.plan_split_limit(256, 6, 4, 12) == 153 == hk.plan_split_limit(256, 5, 4, 12) and hk.plan_split_limit(256, 4, 4, 12) == 122      # six waves count as five


# the first grid point, in grid() order, at which each mutant of the restatement differs from the plan:
# (traversal, occupancy, schedule, num_cus, tiles per wave, count), work, coop_steps, per_frame, wave_log
FIRST = {
    # one CU at four waves per SIMD, one tile per wave, four tiles: the grid is clamped to one workgroup, 4 < 1 * 4 fails and the lean build runs;
    # against the 16 waves of the grid before clamping the launch is short, and so it is with 4 <= 4
    "unclamped": (Cfg(WIDE, 4, 0, 1, 1, 0), 4, 2, 0, 0),
    "le": (Cfg(WIDE, 4, 0, 1, 1, 0), 4, 2, 0, 0),
    # the first short launch of a counting context: the counting build, not the work-sharing one
    "coop_first": (Cfg(WIDE, 4, 0, 1, 1, 1), 1, 2, 0, 0),
    # the first launch with occupancy 6 and schedule 1 that is not short: five waves of the 32 / 8 / 1 build, there is no six-wave one
    "six_schedule_1": (Cfg(WIDE, 6, 1, 1, 0, 0), 1, 0, 0, 0),
    # the very first launch of the grid whose log is on: the threaded builds report blocks * 4 waves although they never log
    "threaded_log_zero": (Cfg(THREADED, 4, 0, 1, 0, 0), 1, 0, 0, 1),
}


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_of_the_restatement_differ_from_the_plan(planned, mutant):
    first, n = None, 0
    for (cfg, work, coop_steps, per_frame, wave_log), plan in planned:
        if as_plan(launch_persistent_kernel(cfg, work, coop_steps, per_frame, bool(wave_log), mutant)) != plan:
            n += 1
            if first is None:
                first = (cfg, work, coop_steps, per_frame, wave_log)
    assert first == FIRST[mutant], (mutant, first, n)
