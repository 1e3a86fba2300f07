"""The closest-hit walks of device_core.hpp, compiled for the host (tools/host_kernel.cpp hk_hit: closest_hit_threaded, closest_hit_ordered,
closest_hit_wide<true> over the tree of wide_tree = 1 and of wide_tree = 2), on every (scene, class) pair of tests/ray_cases.py against the oracle's
hit() -- t bit for bit and the object index, no tolerance -- and the proof, on the oracle and the inputs alone, that every class reaches the edge it is
named for.  No GPU: tests/test_gpu_rays.py sends the same pairs through dr_kat_hit and dr_kat_trace only after they have all returned here.

The corner the far scenes reach ("the leaf-entry rule"): where a coordinate is 2^20, floats step by more than the 0.01 the reference
pads its leaf boxes with, and a leaf's computed box entry can exceed the t of its primitive by an ulp.  grid_mixed / long_short ray 2867 (o = (-2^20, -0.0504,
0.0057), d = (2^18, 0, 0)): object 80, 229th leaf of the reference's order, t = 3.99999952; object 146, 903rd leaf, t = 3.99999928 but box entry 3.99999952.
hit() has object 80 when it reaches the other leaf, `entry < best` fails on the equal values, and object 80 is the answer every walk has to give."""
import os
import sys

import numpy as np
import pytest

import ray_cases as rc
import ray_checks as ck

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

WALKS = ((0, 1), (1, 1), (2, 1), (2, 2))          # (traversal, wide_tree): threaded, ordered, wide over the leaf boxes, wide over own bounds
PAIRS = [(stem, cls) for stem in rc.STEMS for cls, _ in rc.PAIRS[stem]]


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


_host_scenes = {}


def host_scene(hk, L):
    if L.stem not in _host_scenes:
        _host_scenes[L.stem] = hk.Scene(L.path)
    return _host_scenes[L.stem]


def pooled(tmp_path_factory, cls):
    """[(loaded scene, o, d, oracle t, oracle idx)] over every scene the class runs on"""
    return [(ck.loaded(stem, tmp_path_factory),) + ck.loaded(stem, tmp_path_factory).case(cls) for stem, c in PAIRS if c == cls]


@pytest.mark.parametrize("stem,cls", PAIRS)
def test_host_walks_return_the_oracles_hits(hk, tmp_path_factory, stem, cls):
    L = ck.loaded(stem, tmp_path_factory)
    o, d, rt, ri = L.case(cls)
    hs = host_scene(hk, L)
    failed = []
    for traversal, tree in WALKS:
        t, idx = hs.hit(o, d, traversal, tree)
        bad = ck.mismatches(t, idx, rt, ri)
        print("%s / %s traversal %d wide_tree %d: %d rays, %d hits, %d differ" % (stem, cls, traversal, tree, len(o), int((rt > 0).sum()), len(bad)))
        if len(bad):
            failed.append("traversal %d wide_tree %d: %d of %d rays differ -- %s" % (traversal, tree, len(bad), len(o), ck.describe(o, d, t, idx, rt, ri, bad)))
    assert not failed, "%s / %s: %s" % (stem, cls, " | ".join(failed))


def test_scene_preconditions(hk, tmp_path_factory):
    info = {stem: host_scene(hk, ck.loaded(stem, tmp_path_factory)).wide_info(2) for stem in rc.STEMS}
    n = {stem: ck.loaded(stem, tmp_path_factory).g.n for stem in rc.STEMS}
    assert info["grid_small"]["wide_own_bounds"] * 2 > n["grid_small"] and info["grid_small"]["wide_own_bounds"] == n["grid_small"]
    # just over half of the leaves: the builder's chosen * 2 >= N edge
    assert n["grid_mixed"] == rc.GRID_MIXED_SMALL + rc.GRID_MIXED_LARGE and info["grid_mixed"]["wide_own_bounds"] == rc.GRID_MIXED_SMALL
    assert 0 <= 2 * info["grid_mixed"]["wide_own_bounds"] - n["grid_mixed"] <= 2
    assert info["stadium"]["wide_depth"] == 17
    assert info["far_refused"]["wide_depth"] == 0 and host_scene(hk, ck.loaded("far_refused", tmp_path_factory)).wide_info(1)["wide_depth"] == 0
    assert info["far_mesh"]["wide_depth"] >= 2
    for stem in ("tiny_2same", "tiny_2", "tiny_3"):                     # a root with unused child slots
        assert info[stem]["wide_nodes"] == 1 and n[stem] < 4
    assert [n[s] for s in ("tiny_2same", "tiny_2", "tiny_3", "tiny_4", "tiny_5", "tiny_6")] == [2, 2, 3, 4, 5, 6]
    g = ck.loaded("planar", tmp_path_factory).g
    assert (g.a[:, 2] == rc.PLANAR_Z).all() and (g.b[:, 2] == rc.PLANAR_Z).all() and (g.c[:, 2] == rc.PLANAR_Z).all()      # zero extent on z at every node
    assert all(len(rc.PAIRS[s]) and ck.loaded(s, tmp_path_factory).g.n <= 2100 for s in rc.STEMS)


def test_graze_reaches_the_cut_and_the_margin(tmp_path_factory):
    near_cut = below = outside = 0
    for stem in ("grid_small", "grid_mixed"):
        L = ck.loaded(stem, tmp_path_factory)
        o, d, rt, ri = L.case("graze")
        o2, d2, aimed = rc.graze_aimed(np.random.default_rng(rc.seed_of(stem, "graze")), L.g, len(o))
        assert np.array_equal(o, o2) and np.array_equal(ck.bits(d), ck.bits(d2))
        hit = (rt > 0) & (L.g.type[ri] == 2)
        a_hit = np.abs(ck.tri_a(L.g, ri[hit], d[hit]))
        near_cut += int(((a_hit >= 1e-4) & (a_hit < 2e-4)).sum())
        below += int((np.abs(ck.tri_a(L.g, aimed, d)) < rc.F(1e-4)).sum())
        small = hit & np.isin(ri, aimed)
        outside += int((ck.outside_own_bounds(L.g, ri[small], o[small], d[small], rt[small]) > 0).sum())
        dl = np.linalg.norm(d.astype(np.float64), axis=1)
        assert dl.min() < 0.3 and dl.max() > 20 and ((dl > 0.6) & (dl < 1.4)).any()
    print("graze: %d accepted nearest hits with |a| in [1e-4, 2e-4), %d rays below the cut, %d accepted hits outside their triangle's own bounds" % (near_cut, below, outside))
    assert near_cut >= 500 and below >= 500 and outside >= 200


def test_shared_edges_and_duplicates_tie_on_t(orc, tmp_path_factory):
    ties = {"shared_edge": 0, "tie": 0}
    for stem, cls, gen in (("grid_small", "shared_edge", rc.shared_edge_pairs), ("grid_mixed", "shared_edge", rc.shared_edge_pairs), ("ties", "tie", rc.tie_pairs)):
        L = ck.loaded(stem, tmp_path_factory)
        o, d, rt, ri = L.case(cls)
        o2, d2, a, b = gen(np.random.default_rng(rc.seed_of(stem, cls)), L.g, len(o))
        assert np.array_equal(ck.bits(o), ck.bits(o2)) and np.array_equal(ck.bits(d), ck.bits(d2)) and (a != b).all()
        ta, tb = ck.pair_t(orc, L.g, a, o, d), ck.pair_t(orc, L.g, b, o, d)
        tie = (ta > 0) & (ck.bits(ta) == ck.bits(tb)) & (ck.bits(rt) == ck.bits(ta))       # the two tie, and on the nearest hit of the ray
        rank = ck.leaf_rank(L.bvh, L.g.n)
        first = np.where(rank[a] < rank[b], a, b)
        third = tie & (ri != a) & (ri != b)               # a third object with the same t, earlier still in the reference's order
        assert (rank[ri[third]] < rank[first[third]]).all()
        assert np.array_equal(ri[tie & ~third], first[tie & ~third]), "the reference keeps the leaf it reaches first"
        print("%s / %s: %d rays whose nearest hit is a tie of two objects on the bits of t (%d of them with a third)" % (stem, cls, int(tie.sum()), int(third.sum())))
        ties[cls] += int(tie.sum())
        if cls == "tie":
            assert (tie & (L.g.type[a] == 0)).any(), "the duplicated sphere ties as well"
            assert np.abs(rank[a][tie] - rank[b][tie]).max() > 20, "tied leaves far apart in the reference's order"
    assert ties["shared_edge"] >= 200 and ties["tie"] >= 200, ties


def test_cap_lands_on_both_sides_of_10000(tmp_path_factory):
    L = ck.loaded("cap", tmp_path_factory)
    o, d, rt, ri = L.case("cap")
    o2, d2, front, T = rc.cap_rays(np.random.default_rng(rc.seed_of("cap", "cap")), L.g, len(o) - len(o) // 4)
    m = len(o2)
    assert np.array_equal(ck.bits(o[:m]), ck.bits(o2)) and np.array_equal(ck.bits(d[:m]), ck.bits(d2))
    values = rc.cap_values()
    assert len(np.unique(values)) == len(values) and values[rc.CAP_KS.index(0)] == 10000.0
    for j, v in enumerate(values):
        sel = T == v
        assert sel.sum() >= 20
        if v < 10000.0:                                   # k < 0 and 9000: the front triangle, at exactly that t
            assert np.array_equal(ck.bits(rt[:m][sel]), ck.bits(T[sel])) and np.array_equal(ri[:m][sel], front[sel]), v
        else:                                             # k >= 0 and 20000: the farther primitive, or a miss -- never the front triangle
            assert ((rt[:m][sel] < 0) | (ri[:m][sel] != front[sel])).all(), v
    sweep = rt[m:]
    assert (sweep > 0).any() and (sweep < 0).any()


def test_on_plane_forms_nan_products(tmp_path_factory):
    for L, o, d, rt, ri in pooled(tmp_path_factory, "on_plane"):
        k = int(ck.nan_plane_products(L.g, o, d).sum())
        tiny = (np.abs(d) > 0) & (np.abs(d) < 2.0 ** -39)
        assert tiny.any(axis=1).sum() >= len(o) // 4                              # 1 / d at and beyond the wide test's 2^60 clamp
        mid = np.abs(d)[tiny & (np.abs(d) >= 2.0 ** -70)]
        assert len(mid) >= len(o) // 4 and (mid < 2.0 ** -60).any() and (mid > 2.0 ** -60).any()
        assert (np.abs(d)[tiny] < 2.0 ** -126).any() and ((np.abs(d)[tiny] >= 2.0 ** -126) & (np.abs(d)[tiny] <= 2.0 ** -100)).any()      # down to denormals
        print("%s / on_plane: %d of %d rays with a NaN plane product" % (L.stem, k, len(o)))
        assert k >= 200, L.stem                             # on every scene of the class, not on their sum


@pytest.mark.parametrize("cls", ["axis", "in_plane", "inside", "long_short"])
def test_hit_fraction_is_neither_all_nor_nothing(tmp_path_factory, cls):
    hits = rays = 0
    for L, o, d, rt, ri in pooled(tmp_path_factory, cls):
        print("%s / %s: %.3f of %d rays hit" % (L.stem, cls, float((rt > 0).mean()), len(o)))
        hits += int((rt > 0).sum()); rays += len(o)
        assert 0.05 < float((rt > 0).mean()) < 0.95, (L.stem, cls)      # on every scene of the class, and on their sum below
        if cls == "axis":
            z = (d == 0).sum(axis=1)
            assert ((z == 1) | (z == 2)).all() and (z == 1).any() and (z == 2).any() and np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all()
        if cls == "in_plane":
            lying = d[:, 2] == 0
            assert lying.sum() > len(o) // 5 and (o[lying, 2] == rc.PLANAR_Z).all() and (~lying).sum() > len(o) // 5
        if cls == "long_short":
            dl = np.linalg.norm(d.astype(np.float64), axis=1)
            assert dl.min() <= 2.0 ** -39 and dl.max() >= 2.0 ** 31
            oa = np.abs(o).max(axis=1)
            for v in rc.LONG_ORIGINS:
                assert (oa == np.float32(v)).any()
    assert 0.05 < hits / rays < 0.95, hits / rays


def test_nonfinite_rays_are_there_and_some_ray_hits(tmp_path_factory):
    hits = 0
    for L, o, d, rt, ri in pooled(tmp_path_factory, "nonfinite"):
        assert np.isnan(d).any() and np.isinf(d).any() and np.isnan(o).any() and np.isinf(o).any() and (d == 0).all(axis=1).any()
        hits += int((rt > 0).sum())
    assert hits >= 1


def test_ray_counts_of_the_chunk_test_return_on_the_host(hk, tmp_path_factory):
    """the rays tests/test_gpu_rays.py sends through the probe's 128-ray chunks, through the host walks first"""
    L = ck.loaded("grid_mixed", tmp_path_factory)
    hs = host_scene(hk, L)
    for n in rc.RAY_COUNTS:
        o, d = rc.mixed_rays(L.g, n)
        assert len(o) == n
        rt, ri = L.orc.kat_hit(o, d)
        assert rt[-1] > 0 and rt[0] > 0, n                 # a kernel that drops the head or the tail of the list drops a HIT
        for traversal, tree in WALKS:
            t, idx = hs.hit(o, d, traversal, tree)
            assert len(ck.mismatches(t, idx, rt, ri)) == 0, (n, traversal, tree)
