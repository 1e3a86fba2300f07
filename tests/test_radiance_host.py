"""dr_trace_radiance compiled for the host (tools/host_kernel.cpp hk_radiance = device_radiance.hpp radiance_ray over trace_path and the host walks)
against a path loop composed from the oracle's functions only -- orc.Scene.kat_hit, kat_bounce, kat_miss, with the generator's position found in
orc.kat_rng_u32's sequence -- on the all-materials scene of tests/shade_cases.py, radiance bit for bit (tests/shade_checks.py's rule: bit patterns,
a NaN asks for a NaN) and bounces exactly.  Also the launch plan's table and the refusals that need no GPU.  tests/test_gpu_radiance.py compares
the GPU with this host build."""
import os
import sys

import numpy as np
import pytest

import radiance_cases as rc
import shade_checks as ck
from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

THREADED, ORDERED, WIDE = 0, 1, 2
PLAIN, PERSISTENT = 0, 1
CUS = 256


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.fixture(scope="module")
def scenes(hk, tmp_path_factory):
    """(the host build's scene, the oracle's -- a scene of this module's own, with its tree built -- and the rays)"""
    rts, tex = ck.files(tmp_path_factory)
    o, d = rc.shading_rays()
    return hk.Scene(rts, tex), rc.oracle_scene(rts, tex), o, d


# what the compared paths reached, over every case of test_radiance_equals_the_oracles_path_loop: judged by the test behind it
reached = {"branches": np.zeros(10, np.int64), "exhausted": 0, "sky": 0, "cases": 0}


@pytest.mark.parametrize("skipped", [False, True], ids=["skip none", "skip 0..7"])
@pytest.mark.parametrize("max_depth", rc.DEPTHS)
@pytest.mark.parametrize("spp", rc.SPPS)
@pytest.mark.parametrize("backtex", rc.BACKGROUNDS, ids=["sky gradient", "backtex"])
def test_radiance_equals_the_oracles_path_loop(scenes, backtex, spp, max_depth, skipped):
    host, oracle, o, d = scenes
    seed, seeds, skip = rc.shading_seeds(len(o), skipped)
    want = rc.oracle_radiance(oracle, o, d, spp, max_depth, rc.BGINT, backtex, seed, seeds, skip)
    got = host.radiance(o, d, spp, max_depth, rc.BGINT, backtex, seed, seeds, skip)
    reached["branches"] += want["branches"]; reached["exhausted"] += want["exhausted"]; reached["sky"] += want["first_miss"]; reached["cases"] += 1
    ck.compare("host radiance backtex %d spp %d depth %d %s" % (backtex, spp, max_depth, "skip" if skipped else "no skip"), {"o": o, "d": d},
               {"radiance": (got["radiance"], want["radiance"]), "bounces": (got["bounces"], want["bounces"])})
    assert np.isfinite(want["radiance"]).all() and (want["bounces"] >= spp).all() and (want["bounces"] <= spp * max_depth).all()


def test_the_compared_paths_reach_every_branch_and_the_exhausted_depth():
    """every branch the oracle's bounce reports (its Branch enum, orc.BRANCHES) and the depth-exhausted ending (result 0) occur among the paths compared
    above; the sky rays miss at once"""
    assert reached["cases"] == 2 * len(rc.SPPS) * len(rc.DEPTHS) * 2, "run behind test_radiance_equals_the_oracles_path_loop, every case of it"
    print("radiance: bounces per branch %s; %d paths ended with their depth exhausted; %d first rays missed" %
          (dict(zip(ck.BR, reached["branches"].tolist())), reached["exhausted"], reached["sky"]))
    assert (reached["branches"] > 0).all(), dict(zip(ck.BR, reached["branches"].tolist()))
    assert reached["exhausted"] > 0 and reached["sky"] >= rc.N_SKY * reached["cases"]


def test_every_walk_and_both_trees_give_the_same_bits(scenes):
    host, _, o, d = scenes
    seed, seeds, skip = rc.shading_seeds(len(o), True)
    ref = host.radiance(o, d, 3, 10, rc.BGINT, -1, seed, seeds, skip, traversal=WIDE, tree=2)
    assert (ref["bounces"] > 3).any()
    for traversal, tree in ((WIDE, 1), (THREADED, 2), (ORDERED, 2)):
        got = host.radiance(o, d, 3, 10, rc.BGINT, -1, seed, seeds, skip, traversal=traversal, tree=tree)
        ck.compare("host radiance traversal %d tree %d" % (traversal, tree), {"o": o, "d": d},
                   {"radiance": (got["radiance"], ref["radiance"]), "bounces": (got["bounces"], ref["bounces"])})


def test_the_seed_rule(scenes):
    """ray i of a call without seeds is ray 0 of a call with seeds[0] = seed + i, also across 2^64; one channel alone is the same channel"""
    host, _, o, d = scenes
    k = np.arange(0, len(o), 37)
    for base in (0, 12345, 2 ** 64 - 5):
        a = host.radiance(o[k], d[k], 2, 10, rc.BGINT, -1, seed=base)
        seeds = (np.arange(len(k), dtype=np.uint64) + np.uint64(base % 2 ** 64))          # (wraps)
        b = host.radiance(o[k], d[k], 2, 10, rc.BGINT, -1, seed=99, seeds=seeds, skip=np.zeros(len(k), np.int32))
        assert len(ck.differing(a["radiance"], b["radiance"])) == 0 and np.array_equal(a["bounces"], b["bounces"])
    only = host.radiance(o[k], d[k], 2, 10, rc.BGINT, -1, seed=base, channels=("bounces",))
    assert list(only) == ["bounces"] and np.array_equal(only["bounces"], a["bounces"])


def test_refusals_of_the_host_build(scenes):
    host, _, o, d = scenes
    o, d = o[:4], d[:4]
    for kw in ({"spp": 0}, {"max_depth": 0}, {"backtex": len(rc.sc.TEXTURES)}, {"skip": np.array([0, 1, -1, 0], np.int32)}, {"channels": ()}):
        with pytest.raises(RuntimeError) as e:
            host.radiance(o, d, **kw)
        assert len(str(e.value)) > 0, kw
    empty = host.radiance(o[:0], d[:0])
    assert empty["radiance"].shape == (0, 3) and empty["bounces"].shape == (0,)


def test_defaults_need_no_gpu():
    import dogeray_amd as dr
    p = dr.DrRadianceParams()
    assert dr.lib().dr_radiance_defaults(p) == 0
    assert (p.spp, p.max_depth, p.background, p.backtex, p.seed) == (1, 10, 1.0, -1, 0)
    assert dr.lib().dr_radiance_defaults(None) == dr.ERR_INVALID and dr.lib().dr_last_error()
    assert dr.lib().dr_abi_version() == 2


def test_the_threshold_is_the_measured_one(hk):
    """profiles/radiance_rate.txt: the constants are the ones the measurement's file names"""
    text = open(os.path.join(ROOT, "profiles", "radiance_rate.txt")).read()
    assert "RADIANCE_PERSISTENT_MIN_RAYS = %d, refill at %d lanes, leaf steps for %d, chunks of %d rays, %d waves per SIMD" % (
        hk.radiance_persistent_min_rays(), hk.radiance_refill_min(), hk.radiance_park(), hk.radiance_chunk(), hk.radiance_occ()) in text


def test_plan_table(hk):
    m, chunk, occ = hk.radiance_persistent_min_rays(), hk.radiance_chunk(), hk.radiance_occ()
    assert 2 ** 10 <= m < 2 ** 31 and chunk in (64, 128) and occ in (4, 5, 6)
    full, per_block = CUS * occ, 4 * chunk
    table = [
        # n, traversal, has wide, force -> kernel, traversal walked, blocks
        (1, WIDE, True, 0, PLAIN, WIDE, 1),
        (256, WIDE, True, 0, PLAIN, WIDE, 1),
        (257, WIDE, True, 0, PLAIN, WIDE, 2),
        (m - 1, WIDE, True, 0, PLAIN, WIDE, (m - 1 + 255) // 256),
        (m, WIDE, True, 0, PERSISTENT, WIDE, min(full, (m + per_block - 1) // per_block)),
        (2 ** 31 - 1, WIDE, True, 0, PERSISTENT, WIDE, full),
        (2 ** 31 - 1, THREADED, True, 0, PLAIN, THREADED, 2 ** 23),
        # the persistent kernel exists for the wide walk over a wide tree only
        (2 ** 30, WIDE, False, 0, PLAIN, THREADED, 2 ** 22),
        (2 ** 30, THREADED, True, 0, PLAIN, THREADED, 2 ** 22),
        (2 ** 30, ORDERED, True, 0, PLAIN, ORDERED, 2 ** 22),
        (2 ** 30, ORDERED, False, 0, PLAIN, ORDERED, 2 ** 22),
        # option radiance_kernel: 1 one ray per lane, 2 the persistent kernel where it exists
        (2 ** 30, WIDE, True, 1, PLAIN, WIDE, 2 ** 22),
        (1, WIDE, True, 2, PERSISTENT, WIDE, 1),
        (per_block, WIDE, True, 2, PERSISTENT, WIDE, 1),
        (per_block + 1, WIDE, True, 2, PERSISTENT, WIDE, 2),
        (1000, WIDE, False, 2, PLAIN, THREADED, 4),
        (1000, THREADED, True, 2, PLAIN, THREADED, 4),
        (1000, ORDERED, True, 2, PLAIN, ORDERED, 4),
    ]
    for n, traversal, has_wide, force, kernel, walked, blocks in table:
        assert hk.radiance_plan(n, traversal, has_wide, CUS, force) == (kernel, walked, blocks), (n, traversal, has_wide, force)
    for cus in (1, 64, 256, 304):
        assert hk.radiance_plan(2 ** 31 - 1, WIDE, True, cus, 0) == (PERSISTENT, WIDE, cus * occ)


def test_context_radiance_judges_numpy_shapes_without_a_gpu():
    """Context.radiance's shape checks (the shared marshaller, dogeray_amd._list_query) raise before a launch: type and message as ever"""
    import dogeray_amd as dr
    ctx = dr.Context.__new__(dr.Context)      # no device behind it: nothing below may reach one
    o = np.zeros((4, 3), np.float32)
    for bad in ((o, o[:3]), (o[:, :2], o), (o.reshape(-1), o.reshape(-1))):
        with pytest.raises(ValueError) as e:
            ctx.radiance(*bad)
        assert str(e.value) == "o and d must both be [n, 3]"
    for kw in (dict(seeds=np.zeros(3, np.uint64)), dict(skip=np.zeros(5, np.int32)), dict(seeds=np.zeros(4, np.uint64), skip=np.zeros((4, 1), np.int32))):
        with pytest.raises(ValueError) as e:
            ctx.radiance(o, o, **kw)
        assert str(e.value) == "seeds and skip must be [n]"
