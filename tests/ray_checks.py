"""What tests/test_rays_host.py and tests/test_gpu_rays.py share beside the cases of tests/ray_cases.py: the scenes of the table loaded once
(oracle scene, geometry, the oracle's hits of every class), the bit comparison of a walk's answer with the oracle's, and plain numpy restatements
of the quantities the edge conditions are stated in (hit_tri's a, aabb2's plane products, the reference's leaf order)."""
import numpy as np

import ray_cases as rc

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


class Loaded:
    """One scene of the table: its file, the oracle's scene and tree, the geometry the classes aim at; rays and oracle hits per class, computed once"""

    def __init__(self, stem, directory):
        from oracle import orc
        self.stem = stem
        self.path = rc.write_scene(stem, directory)
        self.orc = orc.Scene(self.path, None)
        self.bvh = self.orc.build_bvh()
        self.g = rc.Geometry(self.orc, self.bvh)
        self._cases = {}

    def case(self, cls):
        """(o, d, oracle t, oracle index) of the pair (this scene, cls)"""
        if cls not in self._cases:
            o, d = rc.rays(self.stem, cls, self.g)
            t, idx = self.orc.kat_hit(o, d)
            for a in (o, d, t, idx):
                a.setflags(write=False)
            self._cases[cls] = (o, d, t, idx)
        return self._cases[cls]


_loaded = {}


def loaded(stem, tmp_path_factory):
    if stem not in _loaded:
        _loaded[stem] = Loaded(stem, str(tmp_path_factory.mktemp("rays_" + stem)))
    return _loaded[stem]


def mismatches(t, idx, ref_t, ref_idx):
    """indices of the rays whose answer differs from the oracle's in the bits of t or in the object index"""
    return np.nonzero((bits(t) != bits(ref_t)) | (np.asarray(idx) != ref_idx))[0]


def describe(o, d, t, idx, ref_t, ref_idx, bad, limit=3):
    return "; ".join("ray %d o=%r d=%r: oracle (%r, %d), got (%r, %d)" % (k, o[k].tolist(), d[k].tolist(), float(ref_t[k]), int(ref_idx[k]), float(t[k]), int(idx[k]))
                     for k in bad[:limit])


def tri_a(g, tri, d):
    """hit_tri's a = dot(e1, cross(d, e2)) in float32, operation by operation (K:277-313), for rays d against triangles tri"""
    e1, e2 = (g.b[tri] - g.a[tri]).astype(F), (g.c[tri] - g.a[tri]).astype(F)
    d = d.astype(F)
    hx = d[:, 1] * e2[:, 2] - d[:, 2] * e2[:, 1]
    hy = d[:, 2] * e2[:, 0] - d[:, 0] * e2[:, 2]
    hz = d[:, 0] * e2[:, 1] - d[:, 1] * e2[:, 0]
    return (e1[:, 0] * hx + e1[:, 1] * hy) + e1[:, 2] * hz


def outside_own_bounds(g, tri, o, d, t):
    """how far the exact point o + t d (float64) lies outside the own bounds of triangle tri, worst axis (0: inside)"""
    x = o.astype(np.float64) + t.astype(np.float64)[:, None] * d.astype(np.float64)
    v = np.stack([g.a[tri], g.b[tri], g.c[tri]]).astype(np.float64)
    lo, hi = v.min(axis=0), v.max(axis=0)
    return np.maximum(np.maximum(lo - x, x - hi), 0).max(axis=1)


def nan_plane_products(g, o, d, chunk=256):
    """per ray: does aabb2, restated in float32 ((plane - o) * (1 / d), K:244-274), form a NaN product on some leaf box of the scene"""
    lo, hi = g.lo[g.leaf_obj], g.hi[g.leaf_obj]
    out = np.zeros(len(o), bool)
    with np.errstate(all="ignore"):
        inv = (F(1.0) / d.astype(F))
        for k in range(0, len(o), chunk):
            oo, ii = o[k:k + chunk, None, :], inv[k:k + chunk, None, :]
            out[k:k + chunk] = (np.isnan((lo[None] - oo) * ii) | np.isnan((hi[None] - oo) * ii)).any(axis=(1, 2))
    return out


def leaf_rank(bvh, n):
    """rank of every object's leaf in the reference's child-0-first walk (what a tie on t is decided by: the leaf reached first keeps it)"""
    rank = np.full(n, -1)
    stack, r = [0], 0
    while stack:
        k = stack.pop()
        if bvh["end"][k]:
            rank[bvh["under"][k]] = r
            r += 1
        else:
            stack.append(int(bvh["child1"][k])); stack.append(int(bvh["child0"][k]))
    return rank


def pair_t(orc_mod, g, obj, o, d):
    """the oracle's t of ray k against object obj[k] alone (kat_tri / kat_sphere): -1 where it misses"""
    t = np.full(len(o), -1, F)
    tri = g.type[obj] == 2
    if tri.any():
        t[tri] = orc_mod.kat_tri(o[tri], d[tri], g.a[obj[tri]], g.b[obj[tri]], g.c[obj[tri]])
    sph = g.type[obj] == 0
    if sph.any():
        t[sph] = orc_mod.kat_sphere(o[sph], d[sph], g.a[obj[sph]], g.b[obj[sph], 0])
    return t
