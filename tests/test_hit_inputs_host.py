"""The lean persistent build's forms of a hit's inputs (device_prims.hpp HIT_UV_CARRIED, HIT_FETCH_LAZY) against the plain path, on the host build,
word for word: tri_hit's form that hands out the barycentrics, and shade_prepare_hit<carried, lazy> (tools/host_kernel.cpp hk_tri_hit_uv,
hk_tri_barycentrics, hk_hit_inputs).

Inputs: the adversarial ray / triangle sampler of tests/test_margin_lemma.py (ray_cases.graze_pairs with its seven parameter sets: grazing rays, rims and
corners, |d| from 0.3 to 20) and hand-made degenerate pairs (u or v exactly 0 or 1, u + v rounding to 1, -0.0 as a coordinate and as a barycentric).
Every pair the plain tri_hit accepts is compared; none is skipped.  The accepted pairs are counted on the plain tri_hit alone before anything is
compared: at least 100 000 in all and at least 1 000 in each class of shade record.

texco: the plain path interpolates it for every triangle; the lazy forms leave it 0 where the record has no reader for it (no texture, no roughness
texture, no checker flag).  It is compared word for word on the records that read it, must be 0 in the lazy forms on the others, and what it feeds --
the words of ShadeCtx and the emitted radiance -- is compared on every hit."""
import os
import sys

import numpy as np
import pytest

from ray_cases import graze_pairs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

PARAMS = [(0.03, 30.0, 1.0, 15.0), (0.03, 30.0, 20.0, 15.0), (0.2, 8.0, 1.0, 3.0), (0.005, 100.0, 1.3, 50.0), (1.0, 5.0, 1.0, 2.0), (0.05, 2.0, 0.3, 1.0),
          (0.01, 500.0, 1.0, 200.0)]      # tests/test_margin_lemma.py's
MIN_ACCEPTED, MIN_PER_CLASS = 100000, 1000
# classes of shade record: (face normal: file / -20 sentinel) x (smooth flag off / on) x (no texture coordinate reader / texture / checker / roughness texture)
NORMALS, SMOOTH, TEXKIND = ("file", "sentinel"), (0, 1), ("none", "texture", "checker", "rtexture")
CLASSES = [(a, b, c) for a in NORMALS for b in SMOOTH for c in TEXKIND]
MATERIALS = (0, 2, 3, 4, 5, 1)      # the five that scatter and an emissive one (the path ends: `emitted` is compared)
FORMS = ((True, False), (True, True), (False, True), (False, False))      # (carried, lazy) of shade_prepare_hit


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


def degenerate_pairs():
    """Pairs whose barycentrics are exact: the triangle (0, e1, e2) with e1, e2 along two axes and a ray straight down the third through the point
    (x, y) -- u = x, v = y, t = 1 in exact float arithmetic --, in both orientations (the other gives f = -1: a barycentric 0 comes out as -0.0), at
    three scales and with -0.0 among the coordinates."""
    f = np.float32
    half_up = np.nextafter(f(0.5), f(1))
    pts = [(0, 0), (1, 0), (0, 1), (0.5, 0.5), (0.25, 0.75), (-0.0, 0.3), (0.3, -0.0), (-0.0, -0.0), (0.5, 0.5 - 2.0 ** -25), (0.5, half_up), (1, -0.0),
           (2.0 ** -24, 1), (1 - 2.0 ** -24, 2.0 ** -25), (0.125, 0.125), (0, 0.5), (0.5, 0)]
    o, d, v0, e1, e2 = [], [], [], [], []
    for scale in (1.0, 0.25, 8.0):
        for swap in (False, True):
            for neg_zero_origin in (False, True):
                for (x, y) in pts:
                    a, b = np.array([scale, 0, 0], f), np.array([0, scale, 0], f)
                    base = np.array([-0.0, -0.0, -0.0], f) if neg_zero_origin else np.zeros(3, f)
                    v0.append(base); e1.append(b if swap else a); e2.append(a if swap else b)
                    o.append(np.array([f(x) * f(scale), f(y) * f(scale), 1.0], f)); d.append(np.array([-0.0 if neg_zero_origin else 0.0, 0.0, -1.0], f))
    return [np.array(z, f) for z in (o, d, v0, e1, e2)]


@pytest.fixture(scope="module")
def cases(hk):
    """Every pair of the sampler and of degenerate_pairs() that the plain tri_hit accepts, with a shade record per pair: its class by its index."""
    parts = []
    for (edge, dist, dlen, coord) in PARAMS:
        rng = np.random.default_rng(int(edge * 1e4) + int(dist))
        for rep in range(4):
            parts.append(graze_pairs(rng, 60000, edge, dist, dlen, coord))
    parts.append(degenerate_pairs())
    o, d, v0, e1, e2 = [np.ascontiguousarray(np.concatenate([p[k] for p in parts]), np.float32) for k in range(5)]
    n_degenerate = len(parts[-1][0])
    t_plain, t_uv, uv = hk.tri_hit_uv(o, d, v0, e1, e2)
    # ---- the condition, on the plain tri_hit alone, before anything is compared
    acc = np.nonzero(t_plain > 0)[0]
    assert len(acc) >= MIN_ACCEPTED, "the sampler reaches %d accepted pairs" % len(acc)
    assert int((acc >= len(o) - n_degenerate).sum()) >= n_degenerate // 2, "the degenerate pairs are not accepted"
    cls = np.arange(len(acc)) % len(CLASSES)
    per_class = np.bincount(cls, minlength=len(CLASSES))
    assert per_class.min() >= MIN_PER_CLASS, per_class
    # ---- records
    n = len(acc)
    rng = np.random.default_rng(20251)
    prims = np.zeros((n, 12), np.float32)
    prims[:, 0:3] = v0[acc]; prims[:, 3:6] = e1[acc]; prims[:, 6:9] = e2[acc]
    prims = prims.view(np.uint32).copy()
    prims[:, 9] = 2
    sf = np.zeros((n, 32), np.float32)
    sf[:, 0:3] = rng.normal(size=(n, 3))                                   # the file's face normal
    sf[:, 3:12] = rng.normal(size=(n, 9))                                  # n1, n2, n3
    sf[:, 12:18] = rng.uniform(-2, 3, size=(n, 6))                         # t1, t2, t3
    sf[:, 18:21] = rng.uniform(0, 1, size=(n, 3))                          # col
    sf[:, 21] = np.where(rng.integers(0, 2, n) == 0, 0.0, 1.0)            # addional.x
    sf[:, 22] = rng.uniform(0.05, 1.6, n)                                  # addional.y
    normal_kind = np.array([NORMALS.index(CLASSES[c][0]) for c in cls]); smooth = np.array([CLASSES[c][1] for c in cls])
    texkind = np.array([TEXKIND.index(CLASSES[c][2]) for c in cls])
    sf[normal_kind == 1, 2] = -20.0
    sf[(smooth == 1) & (np.arange(n) % 7 == 0), 5] = -20.0                 # n1.z sentinel: the smooth flag is set and not followed
    sw = sf.view(np.uint32).copy()
    sw[:, 23] = np.array(MATERIALS, np.uint32)[(np.arange(n) // len(CLASSES)) % len(MATERIALS)]
    sw[:, 24] = np.where(texkind == 1, np.arange(n) % 2, -1).astype(np.int32).view(np.uint32)
    sw[:, 25] = np.where(texkind == 3, (np.arange(n) + 1) % 2, -1).astype(np.int32).view(np.uint32)
    sw[:, 26] = (smooth | np.where(texkind == 2, 2, 0)).astype(np.uint32)
    sw[:, 27] = 2
    sw[:, 28] = np.arange(n, dtype=np.uint32)
    tex = np.array([[0, 5, 3, 0], [15, 4, 4, 0]], np.int32)                # two textures: 5 x 3 and 4 x 4 texels
    texels = rng.integers(0, 2 ** 32, 31, dtype=np.uint64).astype(np.uint32)
    seed = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    return {"o": o[acc], "d": d[acc], "v0": v0[acc], "e1": e1[acc], "e2": e2[acc], "t_plain": t_plain[acc], "t_uv": t_uv[acc], "uv": uv[acc],
            "t_plain_all": t_plain, "t_uv_all": t_uv, "prims": prims, "shade": sw, "tex": tex, "texels": texels, "seed": seed, "cls": cls,
            "reads_texco": texkind != 0, "n_degenerate": n_degenerate}


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_uv_form_returns_the_plain_t(cases):
    """Check 2: t of the form that hands out u, v equals the plain form's on every pair, accepted or not."""
    assert np.array_equal(words(cases["t_plain_all"]), words(cases["t_uv_all"]))


def test_uv_are_the_words_surface_normal_forms(hk, cases):
    """Check 1, directly: for every accepted pair u, v equal word for word the ux, uy of tri_barycentrics (device_surface.hpp: surface_normal's
    block K:728-745), and by value the texco that the plain surface_normal interpolates from t1 = (0, 0), t2 = (1, 0), t3 = (0, 1), which is (ux, uy)
    up to the sign of a zero."""
    c = cases
    ux_uy = hk.tri_barycentrics(c["o"], c["d"], c["v0"], c["e1"], c["e2"])
    assert np.array_equal(words(ux_uy), words(c["uv"]))
    assert int((np.signbit(c["uv"]) & (c["uv"] == 0)).sum()) > 0, "no barycentric came out as -0.0"
    assert int((c["uv"] == 1).sum()) > 0 and int((c["uv"].sum(axis=1, dtype=np.float32) == 1).sum()) > 0
    shade = c["shade"].copy()
    ident = np.array([0, 0, 1, 0, 0, 1], np.float32).view(np.uint32)
    shade[:, 12:18] = ident
    plain = hk.hit_inputs(c["o"], c["d"], c["t_plain"], c["uv"], c["prims"], shade, c["seed"], form=0, tex=c["tex"], texels=c["texels"])
    finite = np.isfinite(c["uv"]).all(axis=1)
    assert finite.all()
    assert np.array_equal(plain["texco"], c["uv"] + np.float32(0.0))


@pytest.mark.parametrize("carried,lazy", FORMS)
def test_shade_prepare_hit_equals_shade_prepare(hk, cases, carried, lazy):
    """Check 1, through the shade step: shade_prepare_hit<carried, lazy> and shade_prepare agree word for word on alive, the words of ShadeCtx (N,
    front, ocolor, rough, ...), the emitted radiance, the generator's following outputs and -- where the record reads it -- texco, on every accepted
    pair in every class of record."""
    c = cases
    plain = hk.hit_inputs(c["o"], c["d"], c["t_plain"], c["uv"], c["prims"], c["shade"], c["seed"], form=0, tex=c["tex"], texels=c["texels"])
    got = hk.hit_inputs(c["o"], c["d"], c["t_uv"], c["uv"], c["prims"], c["shade"], c["seed"], form=1, carried=carried, lazy=lazy, tex=c["tex"], texels=c["texels"])
    assert plain["alive"].min() == 0 and plain["alive"].max() == 1
    assert np.array_equal(plain["alive"], got["alive"])
    assert np.array_equal(plain["sc"], got["sc"])
    assert np.array_equal(words(plain["emitted"]), words(got["emitted"]))
    assert np.array_equal(plain["next"], got["next"])
    r = c["reads_texco"]
    assert np.array_equal(words(plain["texco"][r]), words(got["texco"][r]))
    if lazy:
        assert not got["texco"][~r].any()
    else:
        assert np.array_equal(words(plain["texco"]), words(got["texco"]))
    # the classes were really different: flipped normals and both facings, textured colours, checker hits
    alive = plain["alive"] == 1
    assert 0 < int(plain["sc"][alive, 14].sum()) < int(alive.sum())


def test_spheres_and_other_types(hk):
    """The forms on primitives that are no triangles (type 0: a sphere; type 7: never hit by a walk, shaded as the plain path shades it): nothing is
    read from u, v, and the lazy forms fetch the primitive record."""
    rng = np.random.default_rng(5)
    n = 4000
    prims = np.zeros((n, 12), np.float32)
    prims[:, 0:3] = rng.uniform(-3, 3, (n, 3)); prims[:, 3] = rng.uniform(0.1, 2, n)
    pw = prims.view(np.uint32).copy()
    pw[:, 9] = np.where(np.arange(n) % 2 == 0, 0, 7)
    sf = np.zeros((n, 32), np.float32)
    sf[:, 0:12] = rng.normal(size=(n, 12)); sf[:, 12:18] = rng.uniform(-2, 3, (n, 6)); sf[:, 18:21] = rng.uniform(0, 1, (n, 3)); sf[:, 22] = rng.uniform(0.05, 1.6, n)
    sw = sf.view(np.uint32).copy()
    sw[:, 23] = np.array(MATERIALS, np.uint32)[np.arange(n) % len(MATERIALS)]
    sw[:, 24] = np.where(np.arange(n) % 3 == 0, 1, -1).astype(np.int32).view(np.uint32)
    sw[:, 25] = np.uint32(0xffffffff)
    sw[:, 26] = (np.arange(n) % 4).astype(np.uint32)
    sw[:, 27] = pw[:, 9]
    o = rng.uniform(-6, 6, (n, 3)).astype(np.float32); d = rng.normal(size=(n, 3)).astype(np.float32)
    t = rng.uniform(0.1, 9, n).astype(np.float32)
    uv = rng.uniform(-1e3, 1e3, (n, 2)).astype(np.float32)      # garbage: a sphere's stash words hold an earlier hit's
    tex = np.array([[0, 5, 3, 0], [15, 4, 4, 0]], np.int32); texels = rng.integers(0, 2 ** 32, 31, dtype=np.uint64).astype(np.uint32)
    seed = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    plain = hk.hit_inputs(o, d, t, uv, pw, sw, seed, form=0, tex=tex, texels=texels)
    for carried, lazy in FORMS:
        got = hk.hit_inputs(o, d, t, uv, pw, sw, seed, form=1, carried=carried, lazy=lazy, tex=tex, texels=texels)
        for k in ("alive", "sc", "next"):
            assert np.array_equal(plain[k], got[k]), (k, carried, lazy)
        assert np.array_equal(words(plain["emitted"]), words(got["emitted"])) and np.array_equal(words(plain["texco"]), words(got["texco"]))
