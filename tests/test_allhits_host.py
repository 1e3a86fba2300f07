"""dr_trace_all_hits on the host build (no GPU): the two walks of device_allhits.hpp (tools/host_kernel.cpp hk_allhits: allhits_threaded over the
walk array, allhits_wide over the 4-way records of both trees) against the definition itself, hk_allhits_brute -- a loop over every leaf record,
no walk --, bit for bit in count and in all K entries of t and object, on every (scene, class) pair of tests/ray_cases.py; the list's properties;
the cases the list exists for (ties, shared edges, rays in the plane); the relation to the closest hit; and the switch that shows the comparison
reaches the margin lemma.  tests/test_allhits_gpu.py compares the GPU with hk_allhits bit for bit.

No ray class is left out of the equality: EXCLUDED is empty and the test asserts it.  Pairs with fewer than ray_cases.N_RAYS rays in the table are
run with N_RAYS."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import ray_cases as rc
import ray_checks as ck

sys.path.insert(0, os.path.join(ROOT, "tools"))

F = np.float32
EXCLUDED = ()      # ray classes left out of the equality with the brute-force definition: none
PAIR_IDS = [(s, c) for s in rc.STEMS for c, _ in rc.PAIRS[s]]
THREADS = 8


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


_host_scenes, _cases = {}, {}


def host_scene(hk, L):
    if L.stem not in _host_scenes:
        _host_scenes[L.stem] = hk.Scene(L.path)
    return _host_scenes[L.stem]


def case(L, cls):
    """(o, d) of the pair: the table's rays, or N_RAYS of the class where the table has fewer"""
    if dict(rc.PAIRS[L.stem]).get(cls, 0) >= rc.N_RAYS:
        return L.case(cls)[:2]
    if (L.stem, cls) not in _cases:
        o, d = rc.rays(L.stem, cls, L.g, rc.N_RAYS)
        o.setflags(write=False); d.setflags(write=False)
        _cases[(L.stem, cls)] = (o, d)
    return _cases[(L.stem, cls)]


def walks_of(hs):
    """(walk, tree): the threaded links, and the 4-way records of both trees where the scene has them"""
    return ((0, 1), (2, 1), (2, 2)) if hs.has_wide else ((0, 1),)


def differing(out, ref):
    bad = out["count"] != ref["count"]
    if "t" in out and out["t"].shape[1]:
        bad = bad | (ck.bits(out["t"]) != ck.bits(ref["t"])).any(axis=1) | (out["object"] != ref["object"]).any(axis=1)
    return np.nonzero(bad)[0]


def tmax_sets(n, ref_max):
    """(name, tmax): NULL, ray_cases.cap_values() in turn, NaN, values <= 0, and -- cutting the list in the middle -- the t of each ray's second listed
    hit and the float below it (10000 where there is none)"""
    caps = np.resize(rc.cap_values(), n).astype(F)
    nonpos = np.resize(np.array([0.0, -0.0, -1.0, -np.inf], F), n)
    second = np.where(ref_max["count"] >= 2, ref_max["t"][:, 1], F(10000)).astype(F)
    return (("NULL", None), ("cap_values", caps), ("NaN", np.full(n, np.nan, F)), ("nonpositive", nonpos), ("second", second),
            ("below_second", np.nextafter(second, F(0))))


@pytest.mark.parametrize("stem,cls", PAIR_IDS)
def test_walks_equal_the_brute_force_definition(hk, tmp_path_factory, stem, cls):
    assert EXCLUDED == () and cls not in EXCLUDED
    L = ck.loaded(stem, tmp_path_factory)
    hs = host_scene(hk, L)
    o, d = case(L, cls)
    n, KM = len(o), hk.allhits_max()
    assert n >= rc.N_RAYS
    rank = ck.leaf_rank(L.bvh, L.g.n)      # object -> slot: the leaf order of the reference's own walk
    ref_max = hs.allhits_brute(o, d, None, KM, 3, nthreads=THREADS)
    failed = []
    for name, tmax in tmax_sets(n, ref_max):
        refs = {}
        for K in (0, 1, 3, KM):
            ref = refs[K] = hs.allhits_brute(o, d, tmax, K, 3, nthreads=THREADS)
            again = hs.allhits_brute(o, d, tmax, K, 3, nthreads=1)
            assert len(differing(again, ref)) == 0, "the definition itself is not deterministic"
            listed = (ref["t"] > 0).sum(axis=1)
            assert np.isfinite(ref["t"]).all() and ((ref["t"] > 0) | (ref["t"] == -1)).all()
            assert (ref["count"] >= listed).all() and np.array_equal(listed, np.minimum(ref["count"], K))
            assert ((ref["object"] >= 0) == (ref["t"] > 0)).all()
            if K > 1:      # keys strictly increasing over the listed entries: (bits of t, slot); so no slot is listed twice
                tb = ck.bits(ref["t"]).astype(np.int64)
                key = tb * (1 << 27) + rank[np.maximum(ref["object"], 0)]
                both = (ref["t"][:, 1:] > 0)
                assert (np.diff(key, axis=1)[both] > 0).all(), "%s / %s tmax %s: keys not strictly increasing" % (stem, cls, name)
            for walk, tree in walks_of(hs):
                out = hs.allhits(o, d, tmax, K, 3, walk, tree, channels=("count", "t", "object") if K else ("count",), nthreads=THREADS)
                bad = differing(out, ref)
                if len(bad):
                    k = bad[0]
                    failed.append("tmax %s K %d walk %d tree %d: %d of %d rays differ, first %d o=%r d=%r count %d, brute %d" %
                                  (name, K, walk, tree, len(bad), n, k, o[k].tolist(), d[k].tolist(), out["count"][k], ref["count"][k]))
        assert np.array_equal(ck.bits(refs[3]["t"]), ck.bits(refs[KM]["t"][:, :3])) and np.array_equal(refs[3]["object"], refs[KM]["object"][:, :3])
        assert np.array_equal(refs[0]["count"], refs[KM]["count"]) and np.array_equal(refs[1]["count"], refs[KM]["count"])
        if name in ("NaN", "nonpositive"):
            assert (refs[KM]["count"] == 0).all()
        # the kinds partition the set
        tri, sph = hs.allhits_brute(o, d, tmax, 0, 1, nthreads=THREADS)["count"], hs.allhits_brute(o, d, tmax, 0, 2, nthreads=THREADS)["count"]
        assert np.array_equal(tri + sph, refs[0]["count"])
        for walk, tree in walks_of(hs):
            for mask, want in ((1, tri), (2, sph)):
                got = hs.allhits(o, d, tmax, 0, mask, walk, tree, channels=("count",), nthreads=THREADS)["count"]
                if not np.array_equal(got, want):
                    failed.append("tmax %s kind mask %d walk %d tree %d: counts differ" % (name, mask, walk, tree))
    assert not failed, "%s / %s: " % (stem, cls) + " | ".join(failed[:6])


def test_the_ties_scene_lists_every_tie(hk, tmp_path_factory):
    """rays through exact copies and coplanar overlaps: both primitives are listed, at the same bits of t, lower slot first"""
    L = ck.loaded("ties", tmp_path_factory)
    hs = host_scene(hk, L)
    o, d, ia, ib = rc.tie_pairs(np.random.default_rng(rc.seed_of("ties", "tie")), L.g, rc.N_RAYS)
    KM = hk.allhits_max()
    rank = ck.leaf_rank(L.bvh, L.g.n)
    tied = 0
    for walk, tree in walks_of(hs):
        out = hs.allhits(o, d, None, KM, 3, walk, tree, nthreads=THREADS)
        tb = ck.bits(out["t"])
        eq = (tb[:, 1:] == tb[:, :-1]) & (out["t"][:, 1:] > 0)
        assert (rank[out["object"][:, 1:]][eq] > rank[out["object"][:, :-1]][eq]).all()
        pair = np.zeros(len(o), bool)      # the aimed-at pair itself, side by side in the list
        for k in range(KM - 1):
            a, b = out["object"][:, k], out["object"][:, k + 1]
            pair |= eq[:, k] & (((a == ia) & (b == ib)) | ((a == ib) & (b == ia)))
        assert (out["count"][pair] >= 2).all()
        tied = int(pair.sum())
        assert tied > len(o) // 4, "only %d of %d rays list their pair as a tie" % (tied, len(o))
    print("ties: %d of %d rays list the pair they were aimed at as a tie" % (tied, len(o)))


def test_a_shared_edge_counts_zero_one_or_two(hk, tmp_path_factory):
    """a ray through a point of an edge (or a vertex) that two triangles share crosses 0, 1 or 2 of the two at t = 1, and every case occurs: why
    Context.contains lets three directions vote"""
    L = ck.loaded("grid_small", tmp_path_factory)
    hs = host_scene(hk, L)
    o, d, ta, tb = rc.shared_edge_pairs(np.random.default_rng(rc.seed_of("grid_small", "shared_edge")), L.g, rc.N_RAYS)
    KM = hk.allhits_max()
    out = hs.allhits(o, d, None, KM, 1, 2, 2, nthreads=THREADS)
    at_edge = ((out["t"] == 1.0) & ((out["object"] == ta[:, None]) | (out["object"] == tb[:, None]))).sum(axis=1)
    at_edge = at_edge[out["count"] <= KM]      # (a longer list may hold the pair beyond its end)
    hist = np.bincount(at_edge, minlength=3)
    print("shared_edge: rays crossing 0 / 1 / 2 of the two triangles at the shared edge: %s" % hist[:3].tolist())
    assert len(hist) == 3 and (hist > 0).all(), hist.tolist()


def test_rays_in_the_plane_of_a_planar_scene(hk, tmp_path_factory):
    """rays lying in the plane of every triangle cross nothing (hit_tri's |a| cut); the grazing ones beside them cross one, two and more"""
    L = ck.loaded("planar", tmp_path_factory)
    hs = host_scene(hk, L)
    o, d = case(L, "in_plane")
    out = hs.allhits(o, d, None, hk.allhits_max(), 3, 2, 2, nthreads=THREADS)
    lying = (d[:, 2] == 0) & (o[:, 2] == F(rc.PLANAR_Z))
    assert lying.sum() > 500 and (out["count"][lying] == 0).all()
    hist = np.bincount(out["count"][~lying], minlength=3)
    print("planar / in_plane: counts of the grazing rays %s" % hist.tolist())
    assert hist[0] > 0 and hist[1] > 0 and hist[2] > 0
    same_t = ck.bits(out["t"][:, 0]) == ck.bits(out["t"][:, 1])      # overlapping triangles of one plane: ties on t
    assert (same_t & (out["count"] >= 2)).sum() > 0


@pytest.mark.parametrize("stem,cls", PAIR_IDS)
def test_the_first_entry_is_not_behind_the_closest_hit(hk, tmp_path_factory, stem, cls):
    """wherever a closest-hit walk of dr_trace_rays reports a hit (at t <= cap), the list has a first entry and its t is <= that t"""
    L = ck.loaded(stem, tmp_path_factory)
    hs = host_scene(hk, L)
    o, d = case(L, cls)
    first = hs.allhits_brute(o, d, None, 1, 3, nthreads=THREADS)
    for traversal, tree in ((0, 1), (1, 1)) + (((2, 1), (2, 2)) if hs.has_wide else ()):
        tr = hs.trace(o, d, None, traversal, tree)
        hit = tr["t"] > 0
        assert (first["count"][hit] >= 1).all() and (first["t"][hit, 0] > 0).all()
        assert (first["t"][hit, 0] <= tr["t"][hit]).all(), "%s / %s traversal %d tree %d" % (stem, cls, traversal, tree)


@pytest.mark.parametrize("cls", ["axis", "inside"])
def test_well_conditioned_rays_start_with_the_closest_hit(hk, tmp_path_factory, cls):
    """grid_small, classes axis and inside: the first entry IS dr_trace_rays' closest hit, bits of t and object; a miss there is an empty list"""
    L = ck.loaded("grid_small", tmp_path_factory)
    hs = host_scene(hk, L)
    o, d = case(L, cls)
    for walk, tree in walks_of(hs):
        out = hs.allhits(o, d, None, 1, 3, walk, tree, nthreads=THREADS)
        tr = hs.trace(o, d, None, 2, 2)
        assert (tr["t"] > 0).sum() >= 200      # (not emptily: a tenth of the `inside` rays of a scene without spheres hit anything)
        assert np.array_equal(ck.bits(out["t"][:, 0]), ck.bits(tr["t"])) and np.array_equal(out["object"][:, 0], tr["object"])
        assert np.array_equal(out["count"] > 0, tr["t"] > 0)


def test_without_the_margin_the_walk_loses_crossings(hk, tmp_path_factory):
    """the wide node step with the ray's margins forced to zero (a switch of the host build) misses crossings of `graze` rays that the brute-force
    definition has: the equality above reaches the margin lemma"""
    lost = {}
    for stem in ("grid_small", "grid_mixed"):
        L = ck.loaded(stem, tmp_path_factory)
        hs = host_scene(hk, L)
        o, d = case(L, "graze")
        ref = hs.allhits_brute(o, d, None, 0, 3, nthreads=THREADS)
        for tree in (1, 2):
            out = hs.allhits(o, d, None, 0, 3, 2, tree, channels=("count",), zero_margin=True, nthreads=THREADS)
            assert (out["count"] <= ref["count"]).all()      # a walk can only lose crossings, never invent one
            lost[(stem, tree)] = int((out["count"] != ref["count"]).sum())
    print("rays with lost crossings at zero margin (scene, tree): %s" % lost)
    assert max(lost.values()) > 0


def test_the_plan_and_the_refusals(hk, tmp_path_factory):
    KM = hk.allhits_max()
    assert KM in (8, 16)
    assert hk.allhits_plan(1000, True)[:2] == (0, 1) and hk.allhits_plan(1000, False) == (0, 0, 4)
    assert hk.allhits_plan(1000, False, force=2)[0] == 0      # the persistent kernel cannot be forced where it does not exist
    m = hk.allhits_persistent_min_rays()
    assert hk.allhits_plan(1000, True, force=2)[0] == 1 and hk.allhits_plan(m, True)[0] == 1 and hk.allhits_plan(m - 1, True)[0] == 0
    assert hk.allhits_plan(m, True, force=1)[0] == 0 and hk.allhits_plan(m, True, num_cus=256)[2] <= 256 * 5
    assert hk.allhits_plan(129, True, force=2)[2] == 1      # no more waves than chunks
    L = ck.loaded("tiny_2", tmp_path_factory)
    hs = host_scene(hk, L)
    o, d = case(L, "axis")
    for bad in (dict(max_hits=-1), dict(max_hits=KM + 1), dict(kind_mask=0), dict(kind_mask=4), dict(max_hits=0, channels=("count", "t"))):
        with pytest.raises(RuntimeError):
            hs.allhits(o, d, **bad)
    assert hs.allhits(o[:0], d[:0])["t"].shape == (0, 4)


def test_context_trace_all_judges_numpy_shapes_without_a_gpu():
    """Context.trace_all's shape checks (the shared marshaller, dogeray_amd._list_query) raise before a launch: type and message as ever"""
    import dogeray_amd as dr
    ctx = dr.Context.__new__(dr.Context)      # no device behind it: nothing below may reach one
    o = np.zeros((4, 3), np.float32)
    for bad in ((o, o[:3]), (o[:, :2], o), (o.reshape(-1), o.reshape(-1))):
        with pytest.raises(ValueError) as e:
            ctx.trace_all(*bad)
        assert str(e.value) == "o and d must both be [n, 3]"
    with pytest.raises(ValueError) as e:
        ctx.trace_all(o, o, np.zeros(3, np.float32))
    assert str(e.value) == "tmax must be [n]"
