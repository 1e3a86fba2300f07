"""Nearest-surface point queries on the host build (no GPU): device_nearest.hpp's two walks against the brute-force minimum over every primitive, bit
for bit (the pruning proof of DESIGN.md 4.18 held to account); nearest_prim against a float64 restatement within the bound k u (d + 2 Lmax) that the
proof derives and the pruning slack uses; pruning really prunes; the rmax contract."""
import os
import sys

import numpy as np
import pytest

import nearest_cases as nc

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import host_kernel as hk  # noqa: E402

F = np.float32
U = 2.0 ** -24
CHANNELS = hk.NEAREST_CHANNELS
WALKS = ((2, 2), (2, 1), (0, 2))      # (walk, wide_tree): the 4-way records of both trees, the threaded links (which no tree mode changes)

_scenes = {}


def scene(stem, tmp_path_factory):
    if stem not in _scenes:
        sc = hk.Scene(nc.write_scene(stem, str(tmp_path_factory.mktemp("nearest_" + stem))))
        _scenes[stem] = (sc, nc.Prims(sc.nearest_prims()), {})
    return _scenes[stem]


def brute(stem, cls, tmp_path_factory):
    """(points, the brute-force answer) of a pair, computed once and frozen"""
    sc, g, cache = scene(stem, tmp_path_factory)
    if cls not in cache:
        p = nc.points(stem, cls, g)
        ref = sc.nearest_brute(p, nthreads=4)
        p.setflags(write=False)
        for a in ref.values():
            a.setflags(write=False)
        cache[cls] = (p, ref)
    return cache[cls]


def differing(out, ref, n):
    bad = np.zeros(n, bool)
    for k in CHANNELS:
        bad |= (out[k].view(np.uint32) != ref[k].view(np.uint32)).reshape(n, -1).any(axis=1)
    return np.nonzero(bad)[0]


def describe(p, out, ref, bad):
    k = int(bad[0])
    return "%d differ; first: query %d p=%r: brute %r, walk %r" % (len(bad), k, p[k].tolist(), {c: ref[c][k].tolist() for c in CHANNELS},
                                                                    {c: out[c][k].tolist() for c in CHANNELS})


PAIR_IDS = [(s, c) for s in nc.STEMS for c in nc.PAIRS[s]]


# ---------------------------------------------------------------------------------------------- 5a
@pytest.mark.parametrize("stem,cls", PAIR_IDS)
def test_walks_equal_brute_force(stem, cls, tmp_path_factory):
    """5a: every walk's answer is the key-minimum over all primitives, bit for bit in every channel"""
    sc, g, _ = scene(stem, tmp_path_factory)
    assert sc.has_wide == (stem not in nc.NO_WIDE)
    p, ref = brute(stem, cls, tmp_path_factory)
    if cls != "bad":
        assert (ref["object"] >= 0).all()      # unbounded queries at finite points always have an answer
    else:
        fin = np.isfinite(p).all(axis=1)
        assert fin.any() and (~fin).any() and ((ref["object"] >= 0) == fin).all()
    for walk, tree in WALKS:
        out = sc.nearest(p, walk=walk, tree=tree, nthreads=4)
        bad = differing(out, ref, len(p))
        assert len(bad) == 0, "walk %d tree %d: %s" % (walk, tree, describe(p, out, ref, bad))


def test_ties_go_to_the_lower_slot(tmp_path_factory):
    """the `ties` scene holds exact copies: a query nearest to a copied primitive answers with the copy of the lower slot, in every walk"""
    sc, g, _ = scene("ties", tmp_path_factory)
    p, ref = brute("ties", "near", tmp_path_factory)
    slot_of = np.full(g.orig.max() + 1, -1); slot_of[g.orig] = np.arange(len(g.orig))
    key = {}
    for s in range(len(g.kind)):
        key.setdefault((int(g.kind[s]), g.a[s].tobytes(), g.b[s].tobytes(), g.c[s].tobytes()), []).append(s)
    lowest = np.arange(len(g.kind))
    for v in key.values():
        lowest[v] = min(v)
    won = slot_of[ref["object"]]
    copied = np.array([len(key[(int(g.kind[s]), g.a[s].tobytes(), g.b[s].tobytes(), g.c[s].tobytes())]) > 1 for s in won])
    assert copied.sum() > 500
    assert (lowest[won] == won).all()


# ---------------------------------------------------------------------------------------------- 5b
worst = {"prim": 0.0, "scene": 0.0}


@pytest.mark.parametrize("stem", nc.STEMS)
def test_nearest_prim_against_float64(stem, tmp_path_factory):
    """5b: |distance_f - distance_64| <= k u (d + 2 Lmax), k = NEAREST_K of DESIGN.md 4.18 -- per primitive (every point against a random primitive and
    against the winner), and the scene's float64 brute-force minimum against the returned distance"""
    sc, g, _ = scene(stem, tmp_path_factory)
    k = hk.nearest_k()
    assert k == 32
    rng = np.random.default_rng([nc.STEMS.index(stem), 33])
    for cls in nc.PAIRS[stem]:
        if cls == "bad":
            continue
        p, ref = brute(stem, cls, tmp_path_factory)
        n = len(p)
        for slot in (g.cand[rng.integers(0, len(g.cand), n)], None):
            if slot is None:
                slot_of = np.full(g.orig.max() + 1, -1); slot_of[g.orig] = np.arange(len(g.orig))
                slot = slot_of[ref["object"]]
            d2, q, uv = hk.nearest_prim(g.kind[slot], g.a[slot], g.b[slot], g.c[slot], p)
            assert np.isfinite(d2).all() and np.isfinite(q).all() and np.isfinite(uv).all()
            d64 = nc.prim_distance64(g, slot, p)
            bound = k * U * (d64 + 2 * g.lmax)
            err = np.abs(np.sqrt(d2.astype(np.float64)) - d64)
            ratio = float(np.max(err / bound))
            worst["prim"] = max(worst["prim"], ratio)
            assert ratio <= 1.0, "%s/%s: worst |distance_f - distance_64| is %.3f of the bound" % (stem, cls, ratio)
            # the returned point lies at the returned distance, and on the primitive, within the same bound (+ the rounding of q = p + x at q's size)
            dq = np.linalg.norm(q.astype(np.float64) - p.astype(np.float64), axis=1)
            slack = bound + 2 * U * (np.abs(p).max(axis=1) + np.abs(q).max(axis=1)) * np.sqrt(3)
            assert (np.abs(dq - d64) <= 2 * slack).all()
            assert (nc.prim_distance64(g, slot, q) <= 2 * slack).all()
        # the scene's minimum in float64, over every primitive
        d_min = np.full(n, np.inf)
        for s0 in range(0, len(g.cand), 64):
            sl = g.cand[s0:s0 + 64]
            d_min = np.minimum(d_min, nc.prim_distance64(g, sl[None, :], p[:, None, :]).min(axis=1))
        bound = k * U * (d_min + 2 * g.lmax)
        ratio = float(np.max(np.abs(ref["distance"].astype(np.float64) - d_min) / bound))
        worst["scene"] = max(worst["scene"], ratio)
        assert ratio <= 1.0, "%s/%s: the returned distance is %.3f of the bound off the float64 minimum" % (stem, cls, ratio)
    print("worst ratio to k u (d + 2 Lmax), k = %d, so far: per primitive %.4f, scene minimum %.4f" % (k, worst["prim"], worst["scene"]))


def test_nearest_prim_corners():
    """degenerate triangles give the distance to the segment or point they are; a sphere's centre; kinds and radii that never answer"""
    one = lambda kind, a, b, c, p: [x[0] for x in hk.nearest_prim([kind], np.array([a], F), np.array([b], F), np.array([c], F), np.array([p], F))]
    d2, q, uv = one(1, (1, 2, 3), (0, 0, 0), (0, 0, 0), (1, 2, 7))                  # a point
    assert d2 == 16 and q.tolist() == [1, 2, 3]
    d2, q, uv = one(1, (0, 0, 0), (0, 0, 0), (4, 0, 0), (1, 3, 0))                  # a zero edge: the segment (0,0,0)-(4,0,0)
    assert d2 == 9 and q.tolist() == [1, 0, 0]
    d2, q, uv = one(1, (0, 0, 0), (40, 0, 0), (-25, 0, 0), (-30, 0, 2))             # collinear: the segment (-25,0,0)-(40,0,0)
    assert d2 == 29 and q.tolist() == [-25, 0, 0]
    d2, q, uv = one(1, (0, 0, 0), (4, 0, 0), (0, 4, 0), (1, 1, -3))                 # the face
    assert d2 == 9 and q.tolist() == [1, 1, 0] and uv.tolist() == [0.25, 0.25]
    d2, q, uv = one(1, (0, 0, 0), (4, 0, 0), (0, 4, 0), (4, 4, 0))                  # the far edge's midpoint
    assert d2 == 8 and q.tolist() == [2, 2, 0] and uv.tolist() == [0.5, 0.5]
    d2, q, uv = one(0, (1, 1, 1), (2, 0, 0), (0, 0, 0), (1, 1, 1))                  # a sphere's centre
    assert d2 == 4 and q.tolist() == [3, 1, 1] and uv.tolist() == [0, 0]
    d2, q, uv = one(0, (1, 1, 1), (2, 0, 0), (0, 0, 0), (1, 1, 6))
    assert d2 == 9 and q.tolist() == [1, 1, 3]
    for kind, r in ((2, 1.0), (3, 1.0), (0, -1.0), (0, float("nan"))):            # WALK_KIND_NONE, a negative or NaN radius: never a candidate
        assert np.isinf(one(kind, (0, 0, 0), (r, 0, 0), (0, 1, 0), (1, 1, 1))[0])
    rng = np.random.default_rng(34)
    n = 20000
    a = (rng.normal(size=(n, 3)) * np.exp2(rng.integers(-20, 21, (n, 1)))).astype(F)
    e = (rng.normal(size=(n, 3)) * np.exp2(rng.integers(-30, 25, (n, 1)))).astype(F)
    lam = rng.normal(size=(n, 1)).astype(F)
    b = np.where((np.arange(n) % 3 == 0)[:, None], 0, e).astype(F)
    c = np.where((np.arange(n) % 3 == 1)[:, None], e * lam, np.where((np.arange(n) % 3 == 2)[:, None], e, 0)).astype(F)
    p = (a + rng.normal(size=(n, 3)) * np.exp2(rng.integers(-30, 31, (n, 1)))).astype(F)
    p[::7] = a[::7]
    d2, q, uv = hk.nearest_prim(np.ones(n, np.int32), a, b, c, p)
    assert np.isfinite(d2).all() and np.isfinite(q).all() and np.isfinite(uv).all() and (d2 >= 0).all()


# ---------------------------------------------------------------------------------------------- 5c
def test_pruning_prunes(tmp_path_factory):
    """5c: on grid_mixed / near the records visited, summed, are strictly fewer than queries x records, for both trees and both walks"""
    sc, g, _ = scene("grid_mixed", tmp_path_factory)
    p, _ = brute("grid_mixed", "near", tmp_path_factory)
    for walk, tree in WALKS + ((0, 1),):
        vis = sc.nearest(p, walk=walk, tree=tree, channels=("d2",), want_visits=True, nthreads=4)["visits"]
        rec = sc.nearest_records(walk, tree)
        print("grid_mixed / near, walk %d tree %d: %.1f of %d records per query" % (walk, tree, vis.mean(), rec))
        assert 0 < int(vis.sum()) < len(p) * rec
        assert vis.mean() < rec / 4      # and by a wide margin: a slack that grew until nothing is skipped would show here


# ---------------------------------------------------------------------------------------------- 5d
@pytest.mark.parametrize("stem", ("tiny_3", "grid_mixed", "ties", "degenerate", "far_mesh", "far_refused"))
def test_rmax_contract(stem, tmp_path_factory):
    """5d: a hit is returned exactly when its d2 <= fl(rmax rmax); the answers under rmax are the unbounded ones filtered; NaN and negative radii miss"""
    sc, g, _ = scene(stem, tmp_path_factory)
    miss = {"distance": F(-1), "d2": F(0), "object": -1, "material": -1, "point": F(0), "uv": F(0)}
    for cls in ("near", "inside_box", "bad"):
        p, free = brute(stem, cls, tmp_path_factory)
        n = len(p)
        for name, rmax in nc.rmax_sets(free["distance"]).items():
            ref = sc.nearest_brute(p, rmax, nthreads=4)
            if rmax is None:
                assert len(differing(ref, free, n)) == 0
                continue
            with np.errstate(all="ignore"):
                admit = (free["object"] >= 0) & (rmax >= 0) & (free["d2"] <= rmax * rmax)      # (float32 product: fl(rmax rmax); NaN compares false)
            for k in CHANNELS:
                want = np.where(admit.reshape((n,) + (1,) * (free[k].ndim - 1)), free[k], miss[k]).astype(free[k].dtype)
                assert np.array_equal(ref[k].view(np.uint32), want.view(np.uint32)), (name, k)
            if name in ("nan", "negative"):
                assert not admit.any()
            if name in ("inf", "double"):
                assert np.array_equal(admit, free["object"] >= 0)
            if name == "mixed" and cls != "bad":
                assert admit.any() and not admit.all()
            for walk, tree in WALKS:
                out = sc.nearest(p, rmax, walk=walk, tree=tree, nthreads=4)
                bad = differing(out, ref, n)
                assert len(bad) == 0, "rmax %s, walk %d tree %d: %s" % (name, walk, tree, describe(p, out, ref, bad))


def test_context_nearest_judges_numpy_shapes_without_a_gpu():
    """Context.nearest's shape checks (the shared marshaller, dogeray_amd._list_query) raise before the library is called: type and message as ever"""
    import dogeray_amd as dr
    ctx = dr.Context.__new__(dr.Context)      # no device behind it: nothing below may reach one
    p = np.zeros((4, 3), np.float32)
    for bad in (p[:, :2], p.reshape(-1), None):
        with pytest.raises(ValueError) as e:
            ctx.nearest(bad)
        assert str(e.value) == "p must be [n, 3]"
    for rmax in (np.ones(3, np.float32), np.ones((4, 1), np.float32)):
        with pytest.raises(ValueError) as e:
            ctx.nearest(p, rmax=rmax)
        assert str(e.value) == "rmax must be [n]"
