"""Seeded scenes and classes of adversarial rays for the closest-hit walks (device_walk.hpp closest_hit_threaded, closest_hit_ordered,
closest_hit_wide and the lean build's wide_leaf_compute<false> / SignMask / persistent refill), and the table of (scene, class) pairs shared by
tests/test_rays_host.py (no GPU: every pair through the host build of the walks, hk_hit, against the oracle's hit(), and the proof -- on the oracle
and the inputs alone -- that every class reaches the edge it is named for) and tests/test_gpu_rays.py (the same pairs through dr_kat_hit and
dr_kat_trace).

Walk termination.  Every walk is a finite tree walk whatever the float values of a ray are: in the wide walk each step either consumes one record
of the tree (a node or a leaf, each reached through exactly one parent word) or pops one word of the per-lane stack, and a word is pushed only by a
consumed node; the ordered walk likewise consumes a pair or pops a word; the threaded walk follows hit and miss links, which only ever point
forward in the pre-order array, to the terminator.  A NaN or an infinity changes which branch a comparison takes, never the number of records.
The host test runs every case of this file through the host build BEFORE any of it goes to a GPU.

Scenes are written as .rts text with repr() of the float32 values (enough digits to carry them exactly); none is a committed fixture.  The
geometry the ray classes aim at is read back from the oracle (objects(): vertices, centres, radii; build_bvh(): the reference's leaf boxes, own
bounds + 0.01), so a class sees exactly the floats both sides trace against."""
import os

import numpy as np

from scene_fuzz import random_scene, stadium_scene

F = np.float32
HEADER = "*,0.5,-3.0,2.0,0.01,0,0,0,4,45,4,1,1,no,96,64"
CAP_T = 10000.0
CAP_KS = tuple(range(-4, 5))


def _r(x):
    return repr(float(F(x)))


def tri_line(v0, v1, v2, mat=0):
    c = [_r(v) for v in v0] + ["2", "0.8", "0.7", "0.6", "0.3", "0"] + [_r(v) for v in v1] + [str(mat)] + [_r(v) for v in v2]
    return ",".join(c)


def sphere_line(c, r, mat=0):
    return ",".join([_r(v) for v in c] + ["0", "0.8", "0.7", "0.6", "0", "0", _r(r), "0", "0", str(mat)])


def _write(path, lines):
    with open(path, "w") as f:
        f.write("\n".join([HEADER] + lines) + "\n")
    return path


# ------------------------------------------------------------------------------ scenes
GRID_CELL = 1.0 / 64          # ~0.02, a binary fraction: every vertex, every point j/8 along an edge and every difference of two is exact in float32


def _grid_tris(rng, cells, x0, y0, cell=GRID_CELL, zstep=1.0 / 1024, zmax=8):
    """A height field of cells x cells cells from (x0, y0): two triangles per cell sharing the diagonal, heights k * zstep"""
    z = rng.integers(0, zmax + 1, (cells + 1, cells + 1)) * zstep
    P = lambda i, j: (x0 + i * cell, y0 + j * cell, z[i, j])
    out = []
    for i in range(cells):
        for j in range(cells):
            out.append((P(i, j), P(i + 1, j), P(i + 1, j + 1)))
            out.append((P(i, j), P(i + 1, j + 1), P(i, j + 1)))
    return out


def _large_prims(rng, n):
    """Spheres and, every fifth, a large triangle (|e1| + |e2| >= 4.4: never a candidate for own bounds) below and around the grid"""
    lines = []
    for k in range(n):
        if k % 5 != 0:
            c = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-2.5, -0.4)])
            lines.append(sphere_line(c, rng.uniform(0.05, 0.3), int(rng.integers(0, 6))))
            continue
        v0 = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-2.5, -0.3) if k % 7 else rng.uniform(1, 2.5)])      # |v0| < 3.9
        e1 = rng.normal(size=3); e1 *= rng.uniform(2.2, 3.0) / np.linalg.norm(e1)
        e2 = rng.normal(size=3); e2 *= rng.uniform(2.2, 3.0) / np.linalg.norm(e2)
        e1[2] *= 0.2; e2[2] *= 0.2
        e1 *= 2.2 / min(2.2, np.linalg.norm(e1)); e2 *= 2.2 / min(2.2, np.linalg.norm(e2))      # |e1| + |e2| >= 4.4 > the builder's cut max(1, max |v0|)
        lines.append(tri_line(v0, v0 + e1, v0 + e2, int(rng.integers(0, 6))))
    return lines


def scene_grid_small(d):
    rng = np.random.default_rng(101)
    return [_write(os.path.join(d, "grid_small.rts"), [tri_line(*t) for t in _grid_tris(rng, 32, -0.25, -0.25)])]


GRID_MIXED_SMALL, GRID_MIXED_LARGE = 512, 510      # 2 * 512 >= 1022: just over half of the leaves qualify (wide_builder.cpp: chosen * 2 >= N)


def scene_grid_mixed(d):
    rng = np.random.default_rng(102)
    small = [tri_line(*t) for t in _grid_tris(rng, 16, -0.125, -0.125)]
    large = _large_prims(rng, GRID_MIXED_LARGE)
    lines = []
    for k in range(max(len(small), len(large))):      # interleaved in the file
        if k < len(small): lines.append(small[k])
        if k < len(large): lines.append(large[k])
    return [_write(os.path.join(d, "grid_mixed.rts"), lines)]


PLANAR_Z = 0.375


def scene_planar(d):
    rng = np.random.default_rng(103)
    lines = []
    for k in range(300):
        v0 = rng.uniform(-2, 2, 2)
        s = (0.02, 0.3, 1.5)[k % 3]
        a, b = v0 + rng.uniform(-s, s, 2), v0 + rng.uniform(-s, s, 2)
        lines.append(tri_line((v0[0], v0[1], PLANAR_Z), (a[0], a[1], PLANAR_Z), (b[0], b[1], PLANAR_Z), k % 6))
    return [_write(os.path.join(d, "planar.rts"), lines)]


def scene_ties(d):
    """Pairs of primitives that answer a ray with the same t: exact duplicates (first and second copy far apart in the file), coplanar overlapping
    triangles with power-of-two coordinates whose centres lie far apart (so their leaves do), a duplicated sphere; random filler between them"""
    rng = np.random.default_rng(104)
    dup = []
    for k in range(24):
        v0 = np.round(rng.uniform(-2, 2, 3) * 8) / 8
        e1, e2 = np.round(rng.uniform(-1, 1, 3) * 8) / 8, np.round(rng.uniform(-1, 1, 3) * 8) / 8
        if not np.linalg.norm(np.cross(e1, e2)) > 0.05:
            e1, e2 = np.array([0.5, 0, 0.125]), np.array([0, 0.5, 0.25])
        dup.append(tri_line(v0, v0 + e1, v0 + e2, k % 6))
    cop = []
    for k in range(12):                                # two triangles of the plane z = zc, overlapping around (0, 0), centres +-1.5 apart
        zc = -1.0 + 0.25 * k
        cop.append((tri_line((-4, -1, zc), (1, -1, zc), (1, 1.5, zc)), tri_line((4, 1, zc), (-1, 1, zc), (-1, -1.5, zc))))
    sph = [sphere_line((0.5, -0.25, 2.5), 0.5), sphere_line((-1.5, 1.0, -2.0), 0.25)]
    fill = lambda n: [tri_line(*(lambda v0: (v0, v0 + rng.uniform(-0.4, 0.4, 3), v0 + rng.uniform(-0.4, 0.4, 3)))(rng.uniform(-3, 3, 3)), int(rng.integers(0, 6))) for _ in range(n)]
    lines = dup + [c[0] for c in cop] + sph + fill(150) + [c[1] for c in cop] + fill(100) + sph + dup
    return [_write(os.path.join(d, "ties.rts"), lines)]


def scene_tiny_n(d):
    """2 identical objects, then 2 .. 6 objects: the wide tree's root has unused child slots"""
    rng = np.random.default_rng(105)
    t = ((0, 0, 0), (1, 0, 0.25), (0, 1, 0.5))
    out = [_write(os.path.join(d, "tiny_2same.rts"), [tri_line(*t), tri_line(*t)])]
    for n in (2, 3, 4, 5, 6):
        lines = []
        for k in range(n):
            v0 = rng.uniform(-1, 1, 3)
            lines.append(sphere_line(v0, 0.4) if k == 1 else tri_line(v0, v0 + rng.uniform(-1, 1, 3), v0 + rng.uniform(-1, 1, 3)))
        out.append(_write(os.path.join(d, "tiny_%d.rts" % n), lines))
    return out


FAR_SHIFT = float(2 ** 20)
FAR_REFUSED = float(2 ** 44)          # two clusters 2^45 apart: a node extent above 255 * 2^36, which quantise() (wide_builder.cpp) refuses


def scene_far(d):
    rng = np.random.default_rng(106)
    mesh = _grid_tris(rng, 8, FAR_SHIFT, -FAR_SHIFT, cell=2.0, zstep=1.0, zmax=3)       # integer coordinates: exact at 2^20, where floats step by 1 / 8
    a = _write(os.path.join(d, "far_mesh.rts"), [tri_line(*t) for t in mesh] + [sphere_line((FAR_SHIFT + 8, -FAR_SHIFT + 8, 6.0), 2.0)])
    lines = []
    for sx in (-1.0, 1.0):
        for t in _grid_tris(rng, 4, sx * FAR_REFUSED, 0.0, cell=float(2 ** 24), zstep=float(2 ** 22), zmax=3):
            lines.append(tri_line(*t))
    lines.append(sphere_line((FAR_REFUSED, 0.0, float(2 ** 26)), float(2 ** 24)))
    b = _write(os.path.join(d, "far_refused.rts"), lines)
    return [a, b]


def scene_degenerate(d):
    """scene_fuzz.random_scene's zero-area and axis-aligned integer triangles, plus: triangles with a zero-length edge, collinear ones with long edges,
    spheres of radius 0 and tiny"""
    rng = np.random.default_rng(107)
    path = random_scene(rng, 400, os.path.join(d, "degenerate.rts"), duplicates=True, degenerate=True)
    extra = []
    for k in range(60):
        v0 = rng.uniform(-2.5, 2.5, 3)
        e = rng.uniform(-1, 1, 3)
        if k % 3 == 0: extra.append(tri_line(v0, v0, v0 + e))                          # zero-length edge
        elif k % 3 == 1: extra.append(tri_line(v0, v0 + 40 * e, v0 - 25 * e))           # collinear, long
        else: extra.append(sphere_line(v0, (0.0, 1e-6, 1e-3)[k % 9 // 3]))
    with open(path, "a") as f:
        f.write("\n".join(extra) + "\n")
    return [path]


def scene_stadium(d):
    return [stadium_scene(os.path.join(d, "stadium.rts"), 64, 1.5)]


def scene_cap(d):
    """Unit right triangles e1 = (1, 0, 0), e2 = (0, 1, 0) in z = 0, each with a copy 0.5 behind it: for a ray (x, y, T s) + t (0, 0, -s), s a power of two,
    hit_tri's t is T exactly (a = s, f = 1 / s, t = f * (T s))"""
    lines = []
    for k in range(8):
        x, y = float(2 * (k % 4)), float(2 * (k // 4))
        lines.append(tri_line((x, y, 0), (x + 1, y, 0), (x, y + 1, 0)))
        lines.append(tri_line((x, y, -0.5), (x + 1, y, -0.5), (x, y + 1, -0.5)))
    return [_write(os.path.join(d, "cap.rts"), lines)]


SCENES = {"grid_small": scene_grid_small, "grid_mixed": scene_grid_mixed, "planar": scene_planar, "ties": scene_ties, "tiny_n": scene_tiny_n,
          "far": scene_far, "degenerate": scene_degenerate, "stadium": scene_stadium, "cap": scene_cap}


# ------------------------------------------------------------------------------ geometry
class Geometry:
    """What the classes aim at, read from the oracle's scene (after build_bvh): per object type (0 sphere, 2 triangle), a (pos), b (dim), c (rot) --
    a triangle's vertices, a sphere's centre and radius b[:, 0] --; the reference's leaf boxes lo / hi per object; the scene's bounds"""

    def __init__(self, orc_scene, bvh):
        ob = orc_scene.objects()[:orc_scene.n]
        self.n = orc_scene.n
        self.type = ob["type"].copy()
        self.a, self.b, self.c = ob["pos"].astype(F), ob["dim"].astype(F), ob["rot"].astype(F)
        self.tri = np.nonzero(self.type == 2)[0]
        self.sph = np.nonzero(self.type == 0)[0]
        leaf = np.nonzero(bvh["end"][:bvh["used"]] != 0)[0]
        self.lo = np.zeros((self.n, 3), F); self.hi = np.zeros((self.n, 3), F)
        self.lo[bvh["under"][leaf]] = bvh["min"][leaf]; self.hi[bvh["under"][leaf]] = bvh["max"][leaf]
        self.leaf_obj = bvh["under"][leaf]
        fin = np.isfinite(self.lo).all(axis=1) & np.isfinite(self.hi).all(axis=1)
        self.smin, self.smax = self.lo[fin].min(axis=0).astype(np.float64), self.hi[fin].max(axis=0).astype(np.float64)
        self.size = float(np.max(self.smax - self.smin))
        self.ext = np.maximum(np.linalg.norm(self.hi.astype(np.float64) - self.lo.astype(np.float64), axis=1), 1e-3)      # the diagonal of each object's leaf box


def _unit(v):
    return v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-300)


def _box_points(rng, g, idx, spread=0.0):
    """a random point of each object's leaf box, pushed out of it by up to `spread` of its extent"""
    lo, hi = g.lo[idx].astype(np.float64), g.hi[idx].astype(np.float64)
    u = rng.uniform(-spread, 1 + spread, lo.shape)
    return lo + u * (hi - lo)


def _tri_points(rng, g, idx, spread=0.0):
    """a random point of each triangle (barycentric), pushed over its rim by up to `spread`"""
    a, b, c = (x[idx].astype(np.float64) for x in (g.a, g.b, g.c))
    u, v = rng.uniform(-spread, 1 + spread, (len(idx), 1)), rng.uniform(-spread, 1 + spread, (len(idx), 1))
    flip = (u + v > 1) & (rng.random((len(idx), 1)) < 0.8)
    u, v = np.where(flip, 1 - u, u), np.where(flip, 1 - v, v)
    return a + u * (b - a) + v * (c - a)


def _targets(rng, g, n, spread=0.3):
    idx = rng.integers(0, g.n, n)
    p = _box_points(rng, g, idx, spread)
    tri = g.type[idx] == 2
    if tri.any():
        p[tri] = _tri_points(rng, g, idx[tri], spread)
    return idx, p


def _generic(rng, g, n, spread=0.3):
    """rays from around the scene at points on or near its primitives"""
    idx, p = _targets(rng, g, n, spread)
    dirn = _unit(rng.normal(size=(n, 3)))
    dist = g.ext[idx][:, None] * np.exp2(rng.uniform(-3, 5, (n, 1)))      # from next to the primitive to far outside it
    dl = np.exp2(rng.uniform(-2, 4, (n, 1))) * np.maximum(1.0, dist / 512)      # (t stays below hit()'s 10000 in scenes of any size)
    o = p - dirn * dist
    return o.astype(F), (dirn * dl).astype(F)


# ------------------------------------------------------------------------------ ray classes: f(rng, geometry, n) -> (o, d) float32
def axis(rng, g, n):
    """one or two direction components exactly +0 or -0, through a point on or near a primitive; origins inside and outside the scene's boxes"""
    idx, p = _targets(rng, g, n, 0.25)
    d = rng.normal(size=(n, 3)) * np.exp2(rng.uniform(-2, 4, (n, 1))) * np.maximum(1.0, g.ext[idx][:, None] / 16)      # (t stays below hit()'s 10000 in scenes of any size)
    keep = rng.integers(0, 3, n)                       # the component that stays when two are zero
    two = rng.random(n) < 0.4
    zero = np.zeros((n, 3), bool)
    zero[np.arange(n), rng.integers(0, 3, n)] = True
    zero = np.where(two[:, None], np.arange(3)[None, :] != keep[:, None], zero)
    d = np.where(zero, np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0), d)
    s = g.ext[idx][:, None] * np.where(rng.random((n, 1)) < 0.5, rng.uniform(0.0, 0.3, (n, 1)), np.exp2(rng.uniform(0, 5, (n, 1))))      # from inside the boxes / from outside
    o = p - _unit(d) * s
    o = np.where(zero, p, o)                           # (exactly: the ray runs through the point along its zero axes)
    return o.astype(F), d.astype(F)


def on_plane(rng, g, n):
    """an origin coordinate exactly equal to a leaf box's min or max on an axis whose direction component is +-0 ((p - o) * inf = NaN in slab(), 0 * 2^60 -+ m
    in the wide test), or tiny, 2^-70 .. 2^-40 (1 / d beyond the wide test's 2^60 clamp, or close to it); a tenth: smaller still, 2^-126 .. 2^-100 and
    denormal -- without the clamp scale * 2^24 / d overflows there and the folded plane test turns wrong, not merely loose (mutant 2 of the walk's table)"""
    idx = g.leaf_obj[rng.integers(0, len(g.leaf_obj), n)]
    p = _box_points(rng, g, idx, 0.1)
    ax = rng.integers(0, 3, n)
    side = rng.random(n) < 0.5
    plane = np.where(side, g.hi[idx, ax], g.lo[idx, ax])
    d = rng.normal(size=(n, 3)) * np.exp2(rng.uniform(-2, 3, (n, 1))) * np.maximum(1.0, g.ext[idx][:, None] / 16)
    small = np.where(rng.random(n) < 0.5, np.where(rng.random(n) < 0.5, 0.0, -0.0), np.exp2(rng.integers(-70, -39, n).astype(np.float64)) * rng.choice([-1.0, 1.0], n))
    tiny = np.where(rng.random(n) < 0.7, np.exp2(rng.integers(-126, -99, n).astype(np.float64)), np.exp2(rng.integers(-149, -126, n).astype(np.float64))) * rng.choice([-1.0, 1.0], n)
    small = np.where(rng.random(n) < 0.1, tiny, small)
    d[np.arange(n), ax] = small
    s = g.ext[idx][:, None] * np.where(rng.random((n, 1)) < 0.5, rng.uniform(0.0, 0.3, (n, 1)), np.exp2(rng.uniform(0, 5, (n, 1))))
    o = (p - _unit(d) * s).astype(F)
    o[np.arange(n), ax] = plane
    return o, d.astype(F)


def in_plane(rng, g, n):
    """on a planar scene (every vertex in z = c): rays lying in the plane, dz = +-0 and oz = c exactly, and rays crossing it at a grazing angle"""
    zc = float(g.a[g.tri[0], 2])
    idx = g.tri[rng.integers(0, len(g.tri), n)]
    p = _tri_points(rng, g, idx, 0.2)
    lying = rng.random(n) < 0.35
    dirn = _unit(np.concatenate([rng.normal(size=(n, 2)), np.zeros((n, 1))], axis=1))
    dz = np.exp2(rng.uniform(-16, -2, n)) * rng.choice([-1.0, 1.0], n)
    dirn[:, 2] = np.where(lying, np.where(rng.random(n) < 0.5, 0.0, -0.0), dz)
    dl = np.exp2(rng.uniform(-2, 4, (n, 1)))
    o = p - dirn * g.ext[idx][:, None] * np.exp2(rng.uniform(-3, 5, (n, 1)))
    o[:, 2] = np.where(lying, zc, o[:, 2])
    return o.astype(F), (dirn * dl).astype(F)


GRAZE_ALONG_OUT = (1e-6, 1e-2)      # how far outside its triangle a ray along an edge runs, barycentric (log-uniform)


def graze_rays(rng, v0, e1, e2, dist, dlen, along=False):
    """Rays that graze the triangles (v0, e1, e2), one each: aimed at a point of the rim (an edge or a corner, pushed out by up to +-5 %), from ~dist away with
    |d| ~dlen, tilted out of the triangle's plane so that hit_tri's |a| = |d . (e1 x e2)| lands in 0.9 .. 6 x its 1e-4 cut (a third: any tilt).
    along: the rays aimed at an edge run ALONG it, outside the triangle by 1e-6 .. 1e-2 of it (barycentric) over the edge's whole length -- where the edge
    lies in a face of the triangle's own bounds such a ray never enters them, and only the ray's margin keeps the leaf in reach."""
    n = len(v0)
    f = np.float32
    nrm = np.cross(e1.astype(np.float64), e2.astype(np.float64))
    area2 = np.linalg.norm(nrm, axis=1, keepdims=True) + 1e-300
    nrm = nrm / area2
    # a target point around the triangle's rim: barycentrics on an edge or a corner, pushed out by a little
    u = rng.uniform(-0.3, 1.3, (n, 1)); v = rng.uniform(-0.3, 1.3, (n, 1))
    kind = rng.integers(0, 4, (n, 1))
    u = np.where(kind == 0, rng.uniform(-0.05, 0.05, (n, 1)), u)
    v = np.where(kind == 1, rng.uniform(-0.05, 0.05, (n, 1)), v)
    v = np.where(kind == 2, 1 - u + rng.uniform(-0.05, 0.05, (n, 1)), v)
    corner = rng.integers(0, 3, (n, 1))          # kind 3: at a corner
    u = np.where(kind == 3, (corner == 1) + rng.uniform(-0.03, 0.03, (n, 1)), u)
    v = np.where(kind == 3, (corner == 2) + rng.uniform(-0.03, 0.03, (n, 1)), v)
    target = v0 + u * e1 + v * e2
    # direction: in the plane, tilted so that |a| = |d| * 2A * sin(phi) lands around the 1e-4 cut-off (or anywhere, for a third of the cases)
    inplane = e1 * rng.normal(size=(n, 1)) + e2 * rng.normal(size=(n, 1))
    inplane = inplane / (np.linalg.norm(inplane, axis=1, keepdims=True) + 1e-300)
    if along:
        out = np.exp(rng.uniform(np.log(GRAZE_ALONG_OUT[0]), np.log(GRAZE_ALONG_OUT[1]), (n, 1)))      # how far outside, barycentric: from about the walk's own rounding slack up
        u = np.where(kind == 0, -out, u)
        v = np.where(kind == 1, -out, np.where(kind == 2, 1 - u + out, v))
        target = v0 + u * e1 + v * e2
        edge = np.where(kind == 0, e2, np.where(kind == 1, e1, e2 - e1)).astype(np.float64)      # the edge the target lies beside
        elen = np.linalg.norm(edge, axis=1, keepdims=True) + 1e-300
        across = np.cross(nrm, edge / elen)
        drift = rng.uniform(-0.25, 0.25, (n, 1)) * out      # sideways by less than `out` of the triangle over one edge length
        run = (edge / elen + across * drift) * rng.choice([-1.0, 1.0], (n, 1))
        inplane = np.where(kind == 3, inplane, run / np.linalg.norm(run, axis=1, keepdims=True))
    dl = dlen * rng.uniform(0.5, 1.5, (n, 1))
    sinphi = np.clip(1e-4 * rng.uniform(0.9, 6.0, (n, 1)) / (dl * area2), 0, 1)
    sinphi = np.where(rng.integers(0, 3, (n, 1)) == 0, rng.uniform(0, 1, (n, 1)), sinphi) * rng.choice([-1.0, 1.0], (n, 1))
    dirn = inplane * np.sqrt(1 - sinphi ** 2) + nrm * sinphi
    d = (dirn * dl).astype(f)
    t = dist * rng.uniform(0.05, 1.0, (n, 1)) / dl
    o = (target - t * d.astype(np.float64)).astype(f)
    return o, d


def graze_pairs(rng, n, edge, dist, dlen, coord):
    """n adversarial ray / triangle pairs (tests/test_margin_lemma.py): triangle edges ~edge, origin ~dist away, |d| ~dlen, coordinates ~coord"""
    f = np.float32
    v0 = (rng.uniform(-coord, coord, (n, 3))).astype(f)
    e1 = (rng.normal(size=(n, 3)) * edge * rng.uniform(0.2, 1.5, (n, 1))).astype(f)
    e2 = (rng.normal(size=(n, 3)) * edge * rng.uniform(0.2, 1.5, (n, 1))).astype(f)
    # a third of the triangles are cells of a grid, as a height field's are: two edges along the axes (plus a little height), so that the triangle's edges
    # lie IN the faces of its bounds and every overshoot of an edge shows
    grid = rng.integers(0, 3, n) == 0
    gx = np.zeros((n, 3)); gx[:, 0] = edge; gx[:, 2] = rng.normal(size=n) * edge * 0.3
    gy = np.zeros((n, 3)); gy[:, 1] = edge; gy[:, 2] = rng.normal(size=n) * edge * 0.3
    e1 = np.where(grid[:, None], gx, e1).astype(f); e2 = np.where(grid[:, None], gy, e2).astype(f)
    o, d = graze_rays(rng, v0, e1, e2, dist, dlen)
    return o, d, v0, e1, e2


# (distance of the origin, |d|, share of the rays): origins near and far; |d| 0.3 (always below the cut on a 1 / 64 grid: a small share), 1, 20.  The float
# error of hit_tri that the margin has to absorb grows with both, so the far, long rays get the largest share.
GRAZE_COMBOS = ((0.3, 0.3, 0.04), (30.0, 0.3, 0.04), (0.3, 1.0, 0.1), (30.0, 1.0, 0.15), (0.3, 20.0, 0.1), (30.0, 20.0, 0.2), (100.0, 20.0, 0.37))


def graze_aimed(rng, g, n):
    """graze_rays at the scene's small triangles (the ones that can enter the wide tree with their own bounds): (o, d, triangle aimed at)"""
    e1, e2 = g.b - g.a, g.c - g.a
    small = g.tri[np.linalg.norm(e1[g.tri], axis=1) * np.linalg.norm(e2[g.tri], axis=1) < 1e-3]
    o, d, tri = [], [], []
    for dist, dlen, share in GRAZE_COMBOS:
        for along in (False, True):      # half across the rim, half along an edge
            idx = small[rng.integers(0, len(small), int(n * share) // 2)]
            oo, dd = graze_rays(rng, g.a[idx], e1[idx], e2[idx], dist, dlen, along)
            o.append(oo); d.append(dd); tri.append(idx)
    return np.concatenate(o), np.concatenate(d), np.concatenate(tri)


def graze(rng, g, n):
    return graze_aimed(rng, g, n)[:2]


def shared_edge_pairs(rng, g, n):
    """(o, d, triangle, triangle): targets exactly on an edge or a vertex that two of the grid's triangles share -- the point j / 8 along the edge, exact in
    float32 --, from origins whose offset from the target is a small multiple of 2^-8: d = target - o is exact, and the hit is at t = 1"""
    small = g.tri[np.linalg.norm((g.b - g.a)[g.tri], axis=1) * np.linalg.norm((g.c - g.a)[g.tri], axis=1) < 1e-3]
    # edges of the small triangles by their end points: the pairs of triangles that share one
    ends = {}
    for t in small:
        vs = [tuple(g.a[t]), tuple(g.b[t]), tuple(g.c[t])]
        for k in range(3):
            ends.setdefault(tuple(sorted((vs[k], vs[(k + 1) % 3]))), []).append(int(t))
    shared = [(e, ts) for e, ts in ends.items() if len(ts) == 2]
    pick = rng.integers(0, len(shared), n)
    p0 = np.array([shared[k][0][0] for k in pick], np.float64); p1 = np.array([shared[k][0][1] for k in pick], np.float64)
    ta = np.array([shared[k][1][0] for k in pick]); tb = np.array([shared[k][1][1] for k in pick])
    j = rng.integers(0, 9, (n, 1)) / 8.0               # 0 and 1: the shared vertices
    target = p0 + j * (p1 - p0)
    off = rng.integers(-64, 65, (n, 3)) / 256.0
    off[:, 2] = np.abs(off[:, 2]) + 1.0 / 256
    k = np.exp2(rng.integers(0, 5, (n, 1)))            # farther origins: the same direction, 1 .. 16 times as long
    o = target + off * k
    d = -(off * k)
    assert np.array_equal(o.astype(F).astype(np.float64), o) and np.array_equal(d.astype(F).astype(np.float64), d)
    return o.astype(F), d.astype(F), ta, tb


def shared_edge(rng, g, n):
    return shared_edge_pairs(rng, g, n)[:2]


def tie_pairs(rng, g, n):
    """(o, d, object, object) on the scene `ties`: rays through pairs of primitives that are exact copies of each other or lie in one plane and overlap"""
    key = {}
    for i in range(g.n):
        key.setdefault((int(g.type[i]), g.a[i].tobytes(), g.b[i].tobytes(), g.c[i].tobytes()), []).append(i)
    pairs = [(v[0], v[-1]) for v in key.values() if len(v) >= 2]
    flat = [i for i in g.tri if g.a[i, 2] == g.b[i, 2] == g.c[i, 2] and abs(g.a[i, 0]) == 4]      # the coplanar pairs: same z
    byz = {}
    for i in flat:
        byz.setdefault(float(g.a[i, 2]), []).append(int(i))
    pairs += [(v[0], v[1]) for v in byz.values() if len(v) == 2]
    pick = rng.integers(0, len(pairs), n)
    ia = np.array([pairs[k][0] for k in pick]); ib = np.array([pairs[k][1] for k in pick])
    cop = np.isin(ia, flat)
    p = np.where((g.type[ia] == 2)[:, None], _tri_points(rng, g, ia, 0.05), g.a[ia].astype(np.float64))
    # coplanar pairs overlap around the origin of their plane: a point with coordinates on 2^-6, a direction on 2^-4 (everything exact)
    q = np.concatenate([np.round(rng.uniform(-0.9, 0.9, (n, 2)) * 64) / 64, g.a[ia, 2:3].astype(np.float64)], axis=1)
    p = np.where(cop[:, None], q, p)
    dirn = np.where(cop[:, None], np.round(rng.uniform(-2, 2, (n, 3)) * 16) / 16, rng.normal(size=(n, 3)))
    dirn[:, 2] = np.where(cop & (dirn[:, 2] == 0), 1.0, dirn[:, 2])
    s = np.where(cop[:, None], np.exp2(rng.integers(-1, 3, (n, 1)).astype(np.float64)), rng.uniform(0.3, 4.0, (n, 1)))
    o = p - dirn * s
    return o.astype(F), dirn.astype(F), ia, ib


def tie(rng, g, n):
    return tie_pairs(rng, g, n)[:2]


def cap_values():
    """the float32 values of t the class `cap` lands on: 10000 (1 + k 2^-23) for k = -4 .. 4, then 9000 and 20000"""
    return np.array([CAP_T * (1 + k * 2.0 ** -23) for k in CAP_KS] + [9000.0, 20000.0]).astype(F)


def cap_rays(rng, g, n):
    """(o, d, object, value of t): straight down on the front triangles of the scene `cap`, |d| a power of two and the origin T |d| above the triangle, so that
    hit_tri returns T exactly; T runs over cap_values().  The copy 0.5 behind is what a walk that wrongly skipped the front one would return."""
    front = g.tri[g.a[g.tri, 2] == 0]
    T = cap_values()
    idx = front[rng.integers(0, len(front), n)]
    which = np.arange(n) % len(T)
    s = np.exp2(rng.integers(-6, 1, n).astype(np.float64))
    xy = rng.integers(1, 24, (n, 2)) / 64.0            # inside the triangle: u + v < 1
    o = np.concatenate([g.a[idx, :2].astype(np.float64) + xy, (T[which].astype(np.float64) * s)[:, None]], axis=1)
    d = np.concatenate([np.zeros((n, 2)), -s[:, None]], axis=1)
    assert np.array_equal(o.astype(F).astype(np.float64), o)
    return o.astype(F), d.astype(F), idx, T[which]


def cap(rng, g, n):
    """cap_rays, and a sweep of slanted rays whose t is within a few units in the last place of 10000"""
    o, d = cap_rays(rng, g, n - n // 4)[:2]
    m = n // 4
    front = g.tri[g.a[g.tri, 2] == 0]
    p = _tri_points(rng, g, front[rng.integers(0, len(front), m)], 0.0)
    dirn = _unit(rng.normal(size=(m, 3)) * np.array([0.3, 0.3, 1.0]))
    dirn[:, 2] = -np.abs(dirn[:, 2])
    s = np.exp2(rng.integers(-6, 1, (m, 1)).astype(np.float64))
    t = CAP_T * (1 + rng.integers(-8, 9, (m, 1)) * 2.0 ** -23)
    return np.concatenate([o, (p - dirn * s * t).astype(F)]), np.concatenate([d, (dirn * s).astype(F)])


LONG_EXPONENTS = (-40, -30, -20, -12, -6, 0, 6, 12, 20, 30, 31)
LONG_ORIGINS = (2.0 ** 20, 2.0 ** 31, 2.0 ** 59, 2.0 ** 60, 2.0 ** 61, 1e30)


def long_short(rng, g, n):
    """|d| from 2^-40 to 2^31 (beyond wide_ray_margin's 2^30 "tame" guard) at the same geometric ray; and |o| at 2^20 .. 2^61 and 1e30 along one axis, the ray
    running back along that axis through a point on a primitive (exactly: its other two coordinates are the point's)"""
    m = n // 2
    base = m // len(LONG_EXPONENTS)
    o0, d0 = _generic(rng, g, base, 0.15)
    d0 = _unit(d0.astype(np.float64))
    o = [np.tile(o0, (len(LONG_EXPONENTS), 1))]
    d = [np.concatenate([(d0 * 2.0 ** e).astype(F) for e in LONG_EXPONENTS])]
    k = n - len(o[0])
    idx, p = _targets(rng, g, k, 0.15)
    ax = rng.integers(0, 3, k)
    far = np.array(LONG_ORIGINS)[np.arange(k) % len(LONG_ORIGINS)] * rng.choice([-1.0, 1.0], k)
    oo = p.copy()
    oo[np.arange(k), ax] = far
    dd = np.zeros((k, 3))
    dd[np.arange(k), ax] = -far / np.exp2(rng.integers(0, 12, k).astype(np.float64))      # t = 1 .. 2048 or so
    slant = rng.random(k) < 0.25                       # a quarter: not exactly along the axis
    dd = np.where(slant[:, None], dd + rng.normal(size=(k, 3)) * np.abs(dd).max(axis=1, keepdims=True) * 1e-3, dd)
    o.append(oo.astype(F)); d.append(dd.astype(F))
    return np.concatenate(o), np.concatenate(d)


def nonfinite(rng, g, n):
    """a NaN or +-inf in one component of d or o, and d = (0, 0, 0) -- the renderer's own 0 * inf on black surfaces produces them --; every eighth ray is left
    as it was, so that the lanes beside a non-finite ray carry ordinary walks"""
    o, d = _generic(rng, g, n, 0.1)
    bad = np.array([np.nan, np.inf, -np.inf], F)[rng.integers(0, 3, n)]
    comp = rng.integers(0, 3, n)
    where = rng.integers(0, 5, n)                      # 0, 1: d; 2, 3: o; 4: d = 0
    touched = np.arange(n) % 8 != 0
    for arr, sel in ((d, where < 2), (o, (where >= 2) & (where < 4))):
        m = sel & touched
        arr[np.nonzero(m)[0], comp[m]] = bad[m]
    z = (where == 4) & touched
    d[z] = np.where(rng.random((int(z.sum()), 3)) < 0.5, F(0.0), F(-0.0))
    return o, d


def inside(rng, g, n):
    """origins inside spheres, on sphere surfaces and on triangles (t ~ 0 against hit_tri's t > EPS): the primitive the ray starts on must not answer"""
    kind = rng.integers(0, 3, n) if len(g.sph) else np.full(n, 2)
    si = g.sph[rng.integers(0, max(len(g.sph), 1), n)] if len(g.sph) else np.zeros(n, int)
    ti = g.tri[rng.integers(0, len(g.tri), n)]
    dirn = _unit(rng.normal(size=(n, 3)))
    c, r = g.a[si].astype(np.float64), g.b[si, 0:1].astype(np.float64)
    p_in = c + dirn * r * rng.uniform(0, 0.98, (n, 1))
    p_on = c + _unit(rng.normal(size=(n, 3))) * r
    p_tri = _tri_points(rng, g, ti, 0.0)
    o = np.where((kind == 0)[:, None], p_in, np.where((kind == 1)[:, None], p_on, p_tri))
    # aimed at some other primitive half of the time
    idx, p = _targets(rng, g, n, 0.1)
    aim = p - o
    d = np.where((rng.random(n) < 0.6)[:, None], aim, rng.normal(size=(n, 3))) * np.exp2(rng.uniform(-2, 2, (n, 1)))
    return o.astype(F), d.astype(F)


CLASSES = {"axis": axis, "on_plane": on_plane, "in_plane": in_plane, "graze": graze, "shared_edge": shared_edge, "tie": tie, "cap": cap,
           "long_short": long_short, "nonfinite": nonfinite, "inside": inside}

# scene file (stem) -> the classes run on it, with the number of rays
N_RAYS = 4000
PAIRS = {
    "grid_small": (("axis", N_RAYS), ("on_plane", N_RAYS), ("graze", 18000), ("shared_edge", N_RAYS), ("nonfinite", N_RAYS)),
    "grid_mixed": (("axis", N_RAYS), ("on_plane", N_RAYS), ("graze", 18000), ("shared_edge", N_RAYS), ("inside", N_RAYS), ("long_short", N_RAYS), ("nonfinite", N_RAYS)),
    "planar": (("in_plane", N_RAYS), ("axis", N_RAYS), ("on_plane", N_RAYS)),
    "ties": (("tie", N_RAYS), ("axis", N_RAYS), ("on_plane", N_RAYS), ("inside", N_RAYS)),
    "tiny_2same": (("axis", 1000), ("long_short", 1000), ("nonfinite", 1000)),      # (no `inside`: a ray that starts on one of two identical triangles hits neither)
    "tiny_2": (("axis", 1000), ("inside", 1000), ("long_short", 1000)),
    "tiny_3": (("axis", 1000), ("inside", 1000), ("on_plane", 1000)),
    "tiny_4": (("axis", 1000), ("inside", 1000), ("nonfinite", 1000)),
    "tiny_5": (("axis", 1000), ("inside", 1000), ("long_short", 1000)),
    "tiny_6": (("axis", 1000), ("inside", 1000), ("on_plane", 1000)),
    "far_mesh": (("axis", N_RAYS), ("on_plane", N_RAYS), ("long_short", N_RAYS)),
    "far_refused": (("axis", N_RAYS), ("long_short", N_RAYS), ("nonfinite", N_RAYS)),
    "degenerate": (("axis", N_RAYS), ("on_plane", N_RAYS), ("inside", N_RAYS), ("long_short", N_RAYS), ("nonfinite", N_RAYS)),
    "stadium": (("axis", N_RAYS), ("on_plane", N_RAYS), ("long_short", N_RAYS), ("nonfinite", N_RAYS)),
    "cap": (("cap", N_RAYS),),
}
SCENE_OF_STEM = {"tiny_2same": "tiny_n", "tiny_2": "tiny_n", "tiny_3": "tiny_n", "tiny_4": "tiny_n", "tiny_5": "tiny_n", "tiny_6": "tiny_n",
                 "far_mesh": "far", "far_refused": "far"}
STEMS = tuple(PAIRS)


def write_scene(stem, d):
    """the .rts of `stem` written into directory d: its path"""
    for p in SCENES[SCENE_OF_STEM.get(stem, stem)](str(d)):
        if os.path.basename(p) == stem + ".rts":
            return p
    raise KeyError(stem)


def seed_of(stem, cls):
    return [STEMS.index(stem), sorted(CLASSES).index(cls), 20]


def rays(stem, cls, g, n=None):
    """the rays of the pair (stem, cls): (o, d), float32 [n, 3] each"""
    n = dict(PAIRS[stem])[cls] if n is None else n
    o, d = CLASSES[cls](np.random.default_rng(seed_of(stem, cls)), g, n)
    return np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)


def mixed_rays(g, n, salt=None):
    """n rays of one mixed class (a bit of axis, on_plane, long_short, nonfinite and inside each): for the ray counts around the probe's 128-ray chunks.
    salt: MIXED_SALT[n], chosen so that on grid_mixed the last ray of every count HITS (tests/test_rays_host.py asserts it on the oracle): a kernel that
    drops the tail of the list cannot pass for a miss."""
    rng = np.random.default_rng([n, MIXED_SALT.get(n, 0) if salt is None else salt])
    parts = [f(rng, g, n // 5 + 1) for f in (axis, on_plane, long_short, nonfinite, inside)]
    o, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    order = rng.permutation(len(o))[:n]
    return np.ascontiguousarray(o[order], F), np.ascontiguousarray(d[order], F)


RAY_COUNTS = (1, 63, 64, 65, 127, 129, 257, 1000)
MIXED_SALT = {1: 2, 63: 6, 64: 1, 65: 1, 127: 2, 129: 1, 257: 5, 1000: 1}
