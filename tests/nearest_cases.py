"""Seeded classes of query points for the nearest-surface queries (device_nearest.hpp: nearest_prim, nearest_wide, nearest_threaded), on the scenes of
tests/ray_cases.py, and the table of (scene, class) pairs shared by tests/test_nearest_host.py (no GPU: both host walks against the brute-force
minimum, nearest_prim against float64) and tests/test_gpu_nearest.py (Context.nearest against the host build).

A class aims at the primitive RECORDS (tools/host_kernel.py Scene.nearest_prims: v0, e1, e2 / centre, radius in slot order), the floats every walk
measures against.  No scene is a committed fixture."""
import numpy as np

import ray_cases as rc

F = np.float32
N_POINTS = 4000
KIND_SPHERE, KIND_TRIANGLE = 0, 1


def write_scene(stem, d):
    return rc.write_scene(stem, d)


class Prims:
    """the records of a scene (Scene.nearest_prims) and what the classes need of them"""

    def __init__(self, rec):
        self.kind, self.a, self.b, self.c = rec["kind"], rec["a"], rec["b"], rec["c"]
        self.orig, self.material, self.lmax = rec["orig"], rec["material"], rec["lmax"]
        self.tri = np.nonzero(self.kind == KIND_TRIANGLE)[0]
        self.sph = np.nonzero((self.kind == KIND_SPHERE) & (self.b[:, 0] >= 0))[0]
        self.cand = np.concatenate([self.tri, self.sph])
        a64 = self.a.astype(np.float64)
        lo = np.where((self.kind == KIND_TRIANGLE)[:, None], np.minimum(a64, np.minimum(a64 + self.b, a64 + self.c)), a64 - self.b[:, :1].astype(np.float64))
        hi = np.where((self.kind == KIND_TRIANGLE)[:, None], np.maximum(a64, np.maximum(a64 + self.b, a64 + self.c)), a64 + self.b[:, :1].astype(np.float64))
        self.smin, self.smax = lo[self.cand].min(axis=0), hi[self.cand].max(axis=0)
        self.size = float(np.max(self.smax - self.smin))
        self.ext = np.maximum(np.linalg.norm(hi - lo, axis=1), 1e-3)


def _unit(v):
    return v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-300)


def _surface(rng, g, idx):
    """a random point on each primitive idx (float64)"""
    a, b, c = g.a[idx].astype(np.float64), g.b[idx].astype(np.float64), g.c[idx].astype(np.float64)
    u, v = rng.uniform(0, 1, (len(idx), 1)), rng.uniform(0, 1, (len(idx), 1))
    flip = u + v > 1
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    tri = a + u * b + v * c
    sph = a + _unit(rng.normal(size=(len(idx), 3))) * b[:, :1]
    return np.where((g.kind[idx] == KIND_TRIANGLE)[:, None], tri, sph)


def near(rng, g, n):
    """on and within 1e-6 .. 1e-1 (of the primitive's extent, at least 1e-3) of random surface points, on both sides; a tenth exactly on"""
    idx = g.cand[rng.integers(0, len(g.cand), n)]
    s = _surface(rng, g, idx)
    off = np.exp(rng.uniform(np.log(1e-6), np.log(1e-1), (n, 1))) * np.maximum(1.0, g.ext[idx][:, None])
    off = np.where(rng.random((n, 1)) < 0.1, 0.0, off)
    nrm = np.cross(g.b[idx].astype(np.float64), g.c[idx].astype(np.float64))
    dirn = np.where(((g.kind[idx] == KIND_TRIANGLE) & (rng.random(n) < 0.7))[:, None], _unit(nrm) * rng.choice([-1.0, 1.0], (n, 1)), _unit(rng.normal(size=(n, 3))))
    return (s + dirn * off).astype(F)


def _shared_edges(g):
    """(p0, p1, triangle, triangle) of the edges two triangles share, by their end points' floats"""
    v = [g.a, (g.a + g.b).astype(F), (g.a + g.c).astype(F)]
    ends = {}
    for t in g.tri:
        vs = [tuple(x[t].tolist()) for x in v]
        for k in range(3):
            ends.setdefault(tuple(sorted((vs[k], vs[(k + 1) % 3]))), []).append(int(t))
    return [(e[0], e[1], ts[0], ts[1]) for e, ts in ends.items() if len(ts) >= 2 and e[0] != e[1]]


def vertex_edge(rng, g, n):
    """exactly on vertices (v0, fl(v0 + e1), fl(v0 + e2)) and on edge midpoints, and off the midpoints of shared edges along the bisector of the two
    triangles' normals (both signs) -- ties between neighbouring triangles, which the lower slot must win; scenes without triangles: sphere poles"""
    if len(g.tri) == 0:
        idx = g.sph[rng.integers(0, len(g.sph), n)]
        ax = np.eye(3)[rng.integers(0, 3, n)] * rng.choice([-1.0, 1.0], (n, 1))
        return (g.a[idx].astype(np.float64) + ax * g.b[idx, :1]).astype(F)
    idx = g.tri[rng.integers(0, len(g.tri), n)]
    a = g.a[idx]
    v = np.stack([a, (a + g.b[idx]).astype(F), (a + g.c[idx]).astype(F)])      # [3, n, 3], float32 sums as the shared-edge match forms them
    k0, k1 = rng.integers(0, 3, n), rng.integers(0, 3, n)
    p0, p1 = v[k0, np.arange(n)].astype(np.float64), v[k1, np.arange(n)].astype(np.float64)
    what = rng.integers(0, 3, n)
    p = np.where((what == 0)[:, None], p0, 0.5 * (p0 + p1))      # a vertex | an edge midpoint (k0 == k1: the vertex again)
    shared = _shared_edges(g)
    if shared:
        pick = rng.integers(0, len(shared), n)
        q0 = np.array([shared[k][0] for k in pick], np.float64); q1 = np.array([shared[k][1] for k in pick], np.float64)
        ta = np.array([shared[k][2] for k in pick]); tb = np.array([shared[k][3] for k in pick])
        na = _unit(np.cross(g.b[ta].astype(np.float64), g.c[ta].astype(np.float64))); nb = _unit(np.cross(g.b[tb].astype(np.float64), g.c[tb].astype(np.float64)))
        nb = np.where((np.sum(na * nb, axis=1) < 0)[:, None], -nb, nb)
        bis = _unit(na + nb) * rng.choice([-1.0, 1.0], (n, 1))
        j = rng.integers(0, 9, (n, 1)) / 8.0
        off = np.exp2(rng.integers(-12, 1, (n, 1)).astype(np.float64)) * np.linalg.norm(q1 - q0, axis=1, keepdims=True)
        p = np.where((what == 2)[:, None], q0 + j * (q1 - q0) + bis * off, p)
    return p.astype(F)


def inside_box(rng, g, n):
    """uniform in the scene's bounds"""
    return rng.uniform(g.smin, g.smax, (n, 3)).astype(F)


def far(rng, g, n):
    """1e2 .. 1e6 scene sizes (at least 1e2 .. 1e6 units) away from the scene's centre"""
    c = 0.5 * (g.smin + g.smax)
    r = np.exp(rng.uniform(np.log(1e2), np.log(1e6), (n, 1))) * max(1.0, min(g.size, 1e3))
    return (c + _unit(rng.normal(size=(n, 3))) * r).astype(F)


def centre(rng, g, n):
    """sphere centres, exactly, and points inside the spheres"""
    idx = g.sph[rng.integers(0, len(g.sph), n)]
    c, r = g.a[idx].astype(np.float64), g.b[idx, :1].astype(np.float64)
    inside = c + _unit(rng.normal(size=(n, 3))) * r * rng.uniform(0, 1, (n, 1))
    return np.where((rng.random(n) < 0.4)[:, None], c, inside).astype(F)


def bad(rng, g, n):
    """a NaN, +-inf or a 2^31-sized value in one or all components; every eighth point is left ordinary so that its neighbours in a wave walk"""
    p = near(rng, g, n)
    val = np.array([np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 3.0 * 2.0 ** 31], F)[rng.integers(0, 6, n)]
    comp = rng.integers(0, 3, n)
    touched = np.nonzero(np.arange(n) % 8 != 0)[0]
    p[touched, comp[touched]] = val[touched]
    allc = touched[rng.random(len(touched)) < 0.2]
    p[allc] = val[allc, None]
    return p


def tri_distance64(a, b, c, p):
    """distance of p to the triangles (a, a + b, a + c), float64, by the region classification of Ericson (Real-Time Collision Detection 5.1.5), with
    the minimum over the three segments beside it (a zero-area triangle has no face region and leaves NaNs in the classification)"""
    a, b, c, p = (x.astype(np.float64) for x in (a, b, c, p))
    A, B, C = a, a + b, a + c
    with np.errstate(all="ignore"):
        def seg(P0, P1):
            e = P1 - P0
            ee = np.sum(e * e, axis=-1)
            t = np.clip(np.where(ee > 0, np.sum((p - P0) * e, axis=-1) / np.where(ee > 0, ee, 1), 0.0), 0, 1)
            return np.linalg.norm(P0 + t[..., None] * e - p, axis=-1)
        best = np.minimum(seg(A, B), np.minimum(seg(A, C), seg(B, C)))
        ab, ac, ap = B - A, C - A, p - A
        d1, d2 = np.sum(ab * ap, -1), np.sum(ac * ap, -1)
        bp = p - B; d3, d4 = np.sum(ab * bp, -1), np.sum(ac * bp, -1)
        cp = p - C; d5, d6 = np.sum(ab * cp, -1), np.sum(ac * cp, -1)
        va, vb, vc = d3 * d6 - d5 * d4, d5 * d2 - d1 * d6, d1 * d4 - d3 * d2
        face = (va > 0) & (vb > 0) & (vc > 0)
        den = va + vb + vc
        v, w = vb / den, vc / den
        q = A + v[..., None] * ab + w[..., None] * ac
        dface = np.linalg.norm(q - p, axis=-1)
        # the plane distance, where the foot is inside: the same number without the barycentrics' conditioning
        n = np.cross(ab, ac); nn = np.sum(n * n, -1)
        dplane = np.abs(np.sum(ap * n, -1)) / np.sqrt(np.where(nn > 0, nn, 1))
        dface = np.where(face & (nn > 0), np.minimum(dface, np.maximum(dplane, 0)), np.inf)
    return np.minimum(best, np.where(np.isfinite(dface), dface, np.inf))


def prim_distance64(g, slot, p):
    """distance of p[k] to primitive slot[k] (inf: never a candidate)"""
    a, b, c = g.a[slot], g.b[slot], g.c[slot]
    kind = g.kind[slot]
    tri = kind == KIND_TRIANGLE
    d_tri = tri_distance64(a, b, c, p)
    r = b[..., 0].astype(np.float64)
    d_sph = np.abs(np.linalg.norm(p.astype(np.float64) - a.astype(np.float64), axis=-1) - r)
    out = np.where(tri, d_tri, np.where((kind == KIND_SPHERE) & (r >= 0), d_sph, np.inf))
    return out


CLASSES = {"near": near, "vertex_edge": vertex_edge, "inside_box": inside_box, "far": far, "centre": centre, "bad": bad}

_ALL = ("near", "vertex_edge", "inside_box", "far", "bad")
PAIRS = {
    "tiny_2same": _ALL, "tiny_2": _ALL + ("centre",), "tiny_3": _ALL + ("centre",), "tiny_4": _ALL + ("centre",),
    "tiny_5": _ALL + ("centre",), "tiny_6": _ALL + ("centre",),
    "grid_mixed": _ALL + ("centre",), "ties": _ALL + ("centre",), "degenerate": _ALL + ("centre",), "far_mesh": _ALL + ("centre",),
    "far_refused": _ALL + ("centre",),
}
STEMS = tuple(PAIRS)
NO_WIDE = ("far_refused",)      # scenes the wide builder refuses: the threaded links serve them


def points(stem, cls, g, n=N_POINTS):
    rng = np.random.default_rng([STEMS.index(stem), sorted(CLASSES).index(cls), 31])
    return np.ascontiguousarray(CLASSES[cls](rng, g, n), F)


def rmax_sets(distance):
    """name -> rmax array (None: NULL) for queries whose unbounded answer has `distance` (-1: none): the exact distance, one ulp below it, 0, NaN,
    negative, +inf, and a mix of all of them"""
    d = np.where(distance >= 0, distance, F(1.0)).astype(F)
    n = len(d)
    below = np.nextafter(d, F(-1.0)).astype(F)
    sets = {"null": None, "exact": d, "below": below, "zero": np.zeros(n, F), "nan": np.full(n, np.nan, F), "negative": np.full(n, -1.0, F),
            "inf": np.full(n, np.inf, F), "half": (d * F(0.5)).astype(F), "double": (d * F(2.0)).astype(F)}
    pick = np.arange(n) % 8
    mixed = np.choose(pick, [d, below, np.zeros(n, F), np.full(n, np.nan, F), np.full(n, -1.0, F), np.full(n, np.inf, F), d * F(0.5), d * F(2.0)]).astype(F)
    sets["mixed"] = mixed
    return sets


def count_points(g, n, salt=0):
    """n points of a mix of the classes whose LAST one lies on a surface (so that a dropped tail cannot pass for a miss)"""
    rng = np.random.default_rng([n, salt, 32])
    parts = [near(rng, g, n // 4 + 1), inside_box(rng, g, n // 4 + 1), bad(rng, g, n // 4 + 1), far(rng, g, n // 4 + 1)]
    p = np.concatenate(parts)[rng.permutation(sum(len(x) for x in parts))][:n]
    idx = g.cand[rng.integers(0, len(g.cand), 1)]
    p[-1] = _surface(rng, g, idx)[0].astype(F)
    return np.ascontiguousarray(p, F)


def round_trip(g, p, traced_object, distance, nearest_object, k):
    """Points p on a trace's hit positions (traced_object: the object each ray hit) against the nearest query's answer there: (worst ratio of
    |distance - d64| to the bound k u (d64 + 2 Lmax), worst d64 over that bound at d = 0, share of the points whose float64 nearest OBJECT is unique
    beyond the bound, objects that differ among those)"""
    u = 2.0 ** -24
    n = len(p)
    best = np.full(n, np.inf); second = np.full(n, np.inf); who = np.full(n, -1)
    for s0 in range(0, len(g.cand), 64):
        sl = g.cand[s0:s0 + 64]
        d = prim_distance64(g, sl[None, :], p[:, None, :])
        for j in range(len(sl)):
            dj, oj = d[:, j], g.orig[sl[j]]
            better = dj < best
            second = np.where(better, np.where(who != oj, best, second), np.where((who != oj) & (dj < second), dj, second))
            who = np.where(better, oj, who)
            best = np.where(better, dj, best)
    bound = k * u * (best + 2 * g.lmax)
    ratio = float(np.max(np.abs(distance.astype(np.float64) - best) / bound))
    on_surface = float(np.max(best / (k * u * 2 * g.lmax)))
    unique = second - best > 2 * bound
    differ = int(np.sum(unique & (nearest_object != traced_object)))
    return ratio, on_surface, float(unique.mean()), differ, int(np.sum(unique & (who != traced_object)))
