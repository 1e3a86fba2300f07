"""What tests/test_shade_host.py and tests/test_gpu_shade.py share: the oracle's answers on the inputs of tests/shade_cases.py (computed once a
session and never changed), the proof -- on the oracle's output and the inputs alone -- that the inputs reach the branches they were made for, and the
comparisons of an implementation's hooks (an Impl: the host build's hk_kat_* or the GPU's Context.kat_*) with those answers.

Every comparison is on bit patterns, without a tolerance.  NaN: no float output is compared as bits where it is a NaN, because the two sides do not form
it by the same operation on the same hardware -- x86 gives the default NaN with the sign bit set, gfx950 without it -- so a NaN on one side asks for a NaN
(isnan) in the same place on the other.  That rule covers every float output (points, rays, attenuations, colours); in the committed cases none of
them is a NaN on the oracle's side -- kat_miss at m = 0 fetches texel (0, 0) through NaN coordinates and returns its finite colour (check_miss asserts
that), the NaN and infinite inputs of kat_store and kat_tex end in integers -- so there a NaN from an implementation is a mismatch."""
import functools

import numpy as np

import shade_cases as sc
from conftest import SCENEGEN

F32 = np.float32
BR = {name: k for k, name in enumerate(("diffuse", "diffuse_normalised", "mirror", "metal", "glossy_metal", "glossy_diffuse", "glass_cannot", "glass_schlick",
                                        "glass_refract", "emissive"))}


def orc():
    from oracle import orc as o
    return o


class Impl:
    """The seven hooks of one implementation, with Context.kat_*'s signatures and results (both forms on a leading axis of 2)"""

    def __init__(self, name, sample, outside, tex, bounce, miss, camera, store):
        self.name, self.sample, self.outside, self.tex, self.bounce, self.miss, self.camera, self.store = name, sample, outside, tex, bounce, miss, camera, store


# ------------------------------------------------------------------ comparing
def differing(got, want):
    """indices (first axis) of the elements that differ in their bits; a NaN differs from everything but a NaN"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (g.shape, w.shape, g.dtype, w.dtype)
    if g.dtype == np.float32:
        neq = (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))
    else:
        neq = g != w
    if neq.ndim > 1:
        neq = neq.reshape(len(neq), -1).any(axis=1)
    return np.flatnonzero(neq)


def show(v):
    v = np.asarray(v)
    if v.dtype == np.float32:
        return "[" + " ".join("%r (0x%08x)" % (float(x), int(b)) for x, b in zip(v.ravel(), v.ravel().view(np.uint32))) + "]"
    if v.dtype in (np.uint32, np.uint64):
        return "[" + " ".join("0x%x" % int(x) for x in v.ravel()) + "]"
    return str(v.tolist())


def mismatch_report(what, n, bad, inputs, outputs):
    """the first few mismatches: the case's index, its inputs and both outputs; outputs: name -> (got, want)"""
    lines = []
    for i in bad[:4]:
        lines.append("case %d: %s -> %s" % (i, ", ".join("%s %s" % (k, show(v[i])) for k, v in inputs.items()),
                                            ", ".join("%s got %s want %s" % (k, show(g[i]), show(w[i])) for k, (g, w) in outputs.items())))
    return "%s: %d of %d cases differ from the oracle -- %s" % (what, len(bad), n, " | ".join(lines))


def compare(what, inputs, outputs):
    """outputs: name -> (got, want); fails with the first mismatches of all outputs together"""
    n = len(next(iter(outputs.values()))[1])
    bad = np.unique(np.concatenate([differing(g, w) for g, w in outputs.values()]))
    print("%s: %d cases, %d differ" % (what, n, len(bad)))
    assert len(bad) == 0, mismatch_report(what, n, bad, inputs, outputs)


# ------------------------------------------------------------------ samplers
def oracle_words(seeds, nwords):
    """uint32[len(seeds), nwords]: the generator's first outputs for each seed, from the oracle (orc_kat_rng_u32)"""
    L = orc().lib()
    out = np.empty((len(seeds), nwords), np.uint32)
    base, f = out.ctypes.data, L.orc_kat_rng_u32
    for k, s in enumerate(seeds.tolist()):
        f(s, nwords, base + k * nwords * 4)
    return out


def _uniform(x, y):
    """curand_uniform_double of the outputs x, y"""
    z = x.astype(np.uint64) ^ (y.astype(np.uint64) << np.uint64(21))
    return z.astype(np.float64) * 2.0 ** -53 + 2.0 ** -54


def _approx(x, y):
    """the merged loop's 32-bit coordinate: fmaf((float)(y ^ (x >> 21)), 2^-31, -1) -- the product is exact, so one float subtraction rounds as the fma"""
    return (y ^ (x >> np.uint32(21))).astype(F32) * F32(2.0 ** -31) - F32(1)


def _fma32(a, b, c):
    """fmaf(a, b, c) through float64: a * b is exact there; the sum is rounded to double first, which can differ from the fused result only when it lies on
    a float's rounding boundary to within 2^-53 -- of no weight for counting paths"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def candidate(w, sphere):
    """One candidate of the rejection loops from its words w[0 .. 5] (sphere lanes use six, disk lanes four): (its exact squared length as
    rand_in_unit_sphere / rand_in_unit_disk form it, whether they reject it -- l = sqrtf(d2), l * l >= 1 --, the merged loop's approximate squared length)"""
    ux, uy, uz = _uniform(w[0], w[1]), _uniform(w[2], w[3]), _uniform(w[4], w[5])
    one = F32(1)
    x = np.where(sphere, (ux * 2 - 1).astype(F32), ux.astype(F32) * F32(2) - one)
    y = np.where(sphere, (uy * 2 - 1).astype(F32), uy.astype(F32) * F32(2) - one)
    z = np.where(sphere, (uz * 2 - 1).astype(F32), F32(0))
    d2 = x * x + y * y + z * z
    length = np.sqrt(d2)
    xa, ya, za = _approx(w[0], w[1]), _approx(w[2], w[3]), _approx(w[4], w[5])
    d2a = _fma32(ya, ya, xa * xa)
    return d2, length * length >= one, np.where(sphere, _fma32(za, za, d2a), d2a)


def sampler_paths(seed, warm, kind, nwords):
    """A plain restatement of the two rejection loops over the oracle's words, for the states of kind 2 and 3: per state (finished within nwords, words
    consumed by the accepted point's loop, re-entries -- candidates the plain loop rejects although their approximate squared length is below 1 + 2^-16,
    the ones that send a lane of the merged loop back into it --, candidates whose exact squared length lies within 2^-20 of 1, and candidates the plain
    loop ACCEPTS although their approximate squared length is 1 or more: what the 2^-16 of the merged loop's threshold is there for)"""
    n = len(seed)
    words = oracle_words(seed, nwords)
    per = np.where(kind == 3, 6, 4)
    pos = warm.astype(np.int64).copy()
    done = np.zeros(n, bool)
    reentry, inband, tight = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    while True:
        act = np.flatnonzero(~done & (pos + per + 2 <= nwords))
        if len(act) == 0:
            break
        w = [words[act, np.minimum(pos[act] + j, nwords - 1)] for j in range(6)]
        d2, rejected, d2a = candidate(w, kind[act] == 3)
        reentry[act] += rejected & (d2a < F32(1.0 + 2.0 ** -16))
        inband[act] += np.abs(d2 - F32(1)) < F32(2.0 ** -20)
        tight[act] += ~rejected & (d2a >= F32(1))
        pos[act] += per[act]
        done[act[~rejected]] = True
    return done, pos, reentry, inband, tight


@functools.lru_cache(maxsize=None)
def sampler_ref():
    seed, warm, kind = sc.sampler_states()
    point, nxt = orc().kat_sample(seed, warm, kind)
    drawn = np.flatnonzero(kind != 0)
    done, pos, reentry, inband, tight = sampler_paths(seed[drawn], warm[drawn], kind[drawn], 40)
    late = np.flatnonzero(~done)
    if len(late):
        d2, p2, r2, b2, t2 = sampler_paths(seed[drawn][late], warm[drawn][late], kind[drawn][late], 640)
        done[late], pos[late], reentry[late], inband[late], tight[late] = d2, p2, r2, b2, t2
    # the restatement follows the oracle: it consumed as many words as rand_in_unit_sphere / rand_in_unit_disk did
    follow = oracle_words(seed[drawn][:4096], 640)[np.arange(min(4096, len(drawn))), pos[:4096]]
    return {"seed": seed, "warm": warm, "kind": kind, "point": point, "next": nxt, "drawn": drawn, "done": done, "reentry": reentry, "inband": inband,
            "tight": tight, "follow": follow}


def sampler_preconditions():
    r = sampler_ref()
    kind = r["kind"][r["drawn"]]
    assert r["done"].all(), "a state did not accept a point within 640 words"
    assert np.array_equal(r["follow"], r["next"][r["drawn"][:len(r["follow"])], 0]), "the restated loops do not consume the oracle's number of words"
    sphere_reentries, disk_reentries = int(r["reentry"][kind == 3].sum()), int(r["reentry"][kind == 2].sum())
    inband = int(r["inband"].sum())
    tight_sphere, tight_disk = int(r["tight"][kind == 3].sum()), int(r["tight"][kind == 2].sum())
    print("sampler: %d states, %d sphere and %d disk re-entries, %d squared lengths within 2^-20 of 1, %d sphere and %d disk points accepted with an approximate "
          "squared length of 1 or more" % (len(r["seed"]), sphere_reentries, disk_reentries, inband, tight_sphere, tight_disk))
    assert sphere_reentries >= 8 and disk_reentries >= 4 and inband >= 2, (sphere_reentries, disk_reentries, inband)
    # what the 2^-16 of the merged loop's threshold is for (a loop that rejected at 1 would draw another point): the searched states, each of them
    n_searched = len(sc.searched_states()[0])
    assert n_searched >= 4 and (r["tight"][len(r["drawn"]) - n_searched:] >= 1).all() and tight_sphere + tight_disk >= 4, (n_searched, tight_sphere, tight_disk)
    # kinds 0, 2 and 3 inside every wave of the 2^20
    k = r["kind"][:sc.SAMPLER_N].reshape(-1, 64)
    assert all(((k == v).sum(axis=1) > 0).all() for v in (0, 2, 3))
    return sphere_reentries, disk_reentries, inband


def check_sampler(impl):
    sampler_preconditions()
    r = sampler_ref()
    point, nxt = impl.sample(r["seed"], r["warm"], r["kind"])
    inputs = {"seed": r["seed"], "warm": r["warm"], "kind": r["kind"]}
    compare(impl.name + " kat_sample", inputs, {"plain point": (point[0], r["point"]), "plain next": (nxt[0], r["next"]),
                                                "merged point": (point[1], r["point"]), "merged next": (nxt[1], r["next"])})


# ------------------------------------------------------------------ outside_unit
@functools.lru_cache(maxsize=None)
def outside_ref():
    d2 = sc.outside_values()
    return d2, orc().kat_outside(d2)


def check_outside(impl):
    d2, want = outside_ref()
    assert len(d2) == (1 << 19) + 1 + 7
    # the sweep crosses the place where the plain test flips.  (It flips exactly at 1.0: RN(sqrt) of the largest float below 1 is that float again, of
    # the smallest above 1 it is 1 -- so on these values, and on every float, l * l >= 1 agrees with d2 >= 1, and a device square root that is an ulp off
    # is what this comparison would catch, not a missing band.)
    sweep = want[:(1 << 19) + 1]
    assert sweep[0] == 0 and sweep[-1] == 1 and np.array_equal(np.flatnonzero(np.diff(sweep)), [(1 << 18) - 1])
    print("outside_unit: %d values, %d where l * l >= 1 differs from d2 >= 1" % (len(d2), int((sweep != (d2[:(1 << 19) + 1] >= 1)).sum())))
    compare(impl.name + " kat_outside", {"d2": d2}, {"outside": (impl.outside(d2), want)})


# ------------------------------------------------------------------ the scene
_files = {}


def files(tmp_path_factory):
    if not _files:
        _files["rts"], _files["tex"] = sc.write_scene(str(tmp_path_factory.mktemp("shade")), SCENEGEN)
    return _files["rts"], _files["tex"]


@functools.lru_cache(maxsize=None)
def _oracle_scene(rts, tex):
    s = orc().Scene(rts, tex)
    objs = s.objects()[:-1]
    want = sc.scene_objects()
    assert s.n == len(want) == 70
    # the file says what scene_objects() meant: materials, textures, flags
    for got, o in zip(objs, want):
        assert got["type"] == o["type"] and got["mat"] == o["mat"] and got["addional"][0] == o["add_x"] and got["addional"][1] == F32(o["extra"])
        if o["type"] == 2:
            assert got["smooth"] == o["smooth"] and got["tex"] == o["checker"]
            assert got["texnum"] == {"no": -1, "synth_albedo": sc.TEX_ALBEDO, "testtwo": sc.TEX_TWO}[o["tex"]]
            assert got["rtexnum"] == {"no": -1, "synth_rough": sc.TEX_ROUGH}[o["rtex"]]
            assert (got["norm"][2] == -20) == (o["norm"] is None) and (got["n1"][2] == -20) == (o["vn"] is None)
    tex_shapes = [t.shape[:2] for t in s.textures()]
    assert tex_shapes == [(h, w) for _, w, h, _ in sc.TEXTURES], tex_shapes
    return s


def oracle_scene(tmp_path_factory):
    return _oracle_scene(*files(tmp_path_factory))


# ------------------------------------------------------------------ texel fetch
def f2i(x):
    """float -> int as the device functions convert: saturating, NaN -> 0"""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore"):
        t = np.where(np.isnan(x), 0.0, np.clip(x.astype(np.float64), -2147483648.0, 2147483647.0))
    return np.trunc(t).astype(np.int64)


def texel_index(coord, size):
    """the texel an axis coordinate addresses, restated: frac = c - floor(c), floor(frac * size), converted and clamped; and whether frac is a NaN"""
    with np.errstate(invalid="ignore"):
        frac = coord - np.floor(coord)
        i = f2i(np.floor(frac * F32(size)))
    return np.clip(i, 0, size - 1), np.isnan(frac)


@functools.lru_cache(maxsize=None)
def _tex_ref(rts, tex_dir):
    s = _oracle_scene(rts, tex_dir)
    tex, u, v = sc.tex_cases()
    return tex, u, v, s.kat_tex(tex, u, v)


def tex_preconditions(tmp_path_factory):
    s = oracle_scene(tmp_path_factory)
    tex, u, v, rgba = _tex_ref(*files(tmp_path_factory))
    nan_fracs = 0
    for t, img in enumerate(s.textures()):
        h, w = img.shape[:2]
        word = img[..., 0].astype(np.uint32) | img[..., 1].astype(np.uint32) << 8 | img[..., 2].astype(np.uint32) << 16 | img[..., 3].astype(np.uint32) << 24
        sel = tex == t
        i, nan_u = texel_index(u[sel], w)
        j, nan_v = texel_index(v[sel], h)
        # the restated address is the oracle's: it names the texel the oracle returned, for every case
        assert np.array_equal(word[j, i], rgba[sel]), "texture %d: the restated texel address is not the oracle's" % t
        assert {0, w - 1} <= set(np.unique(i).tolist()) and {0, h - 1} <= set(np.unique(j).tolist()), "texture %d: an edge column or row is never fetched" % t
        nan_fracs += int((nan_u | nan_v).sum())
    print("tex: %d fetches, %d with a NaN fractional part" % (len(tex), nan_fracs))
    assert nan_fracs >= 1
    return nan_fracs


def check_tex(impl, tmp_path_factory):
    tex_preconditions(tmp_path_factory)
    tex, u, v, want = _tex_ref(*files(tmp_path_factory))
    compare(impl.name + " kat_tex", {"texture": tex, "u": u, "v": v}, {"texel": (impl.tex(tex, u, v), want)})


# ------------------------------------------------------------------ one bounce
def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def glass_cosine(scene, idx, o, d, t):
    """raycolor's cos_theta for a bounce, restated in float32 from the oracle's own normal (kat_normal): (the dot product before the clamp at 1, front face)"""
    nrm, _ = scene.kat_normal(idx, o, d, t)
    front = _dot(d, nrm) < 0
    nrm = np.where(front[:, None], nrm, nrm * F32(-1))
    with np.errstate(all="ignore"):
        inv = F32(1) / np.sqrt(_dot(d, d))
        unit = d * inv[:, None]
    return _dot(unit * F32(-1), nrm), front


def cannot_refract(cos, ratio):
    """the glass branch's test on a cosine (float32): ratio * (float)sqrt(1 - (double)(cos * cos)) > 1"""
    sin = np.sqrt(1.0 - (cos * cos).astype(np.float64)).astype(F32)
    return F32(ratio) * sin > 1.0


def critical_cosine(ratio=1.5):
    """the largest float32 cosine at which a back face of ratio `ratio` cannot refract"""
    lo, hi = int(F32(0.5).view(np.uint32)), int(F32(0.99).view(np.uint32))
    bits = np.arange(lo, hi, dtype=np.uint32)
    yes = np.flatnonzero(cannot_refract(bits.view(F32), ratio))
    return bits[yes[-1]].view(F32)


def reflectance(cos, ratio):
    """Schlick's approximation as raycolor forms it (float32; the fifth power by squaring)"""
    one, ratio = F32(1), F32(ratio)
    r0 = (one - ratio) / (one + ratio)
    r0 = r0 * r0
    a = one - cos
    r = a
    a = a * a
    a = a * a
    r = r * a
    return r0 + (one - r0) * r


FRONT_RATIO = F32(1.0 / np.float64(F32(1.5)))          # a front face of ir 1.5


def glass_uniform(seed, warm):
    """the uniform number a glass bounce compares its reflectance with: randy() of the generator's first draw after its warm-up, from the oracle's words"""
    w = oracle_words(seed, 8)
    k = np.arange(len(seed))
    return _uniform(w[k, warm], w[k, warm + 1]).astype(F32)


def schlick_rays(scene, k, ob, rng, seed, warm):
    """Front-face rays for glass object k whose reflectance lies within an ulp or two of the uniform number (seed, warm) gives them, on either side: the
    cosine of each is bisected (40 steps) between grazing and normal incidence, the reflectance restated from the oracle's normal at every step"""
    p, n, back, phi, L, dist = sc.schlick_frames(ob, rng)
    target = glass_uniform(seed, warm)
    idx = np.full(len(p), k, np.int32)
    lo, hi = np.full(len(p), 1e-3), np.ones(len(p))                   # reflectance above the target at lo, at or below it at hi
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        o, d, t = sc.rays_at(p, n, mid, back, phi, L, dist)
        raw, _ = glass_cosine(scene, idx, o, d, t)
        above = reflectance(np.minimum(raw, F32(1)), FRONT_RATIO) > target
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    return sc.rays_at(p, n, np.where(np.arange(len(p)) % 2 == 0, lo, hi), back, phi, L, dist)


def ulps_from(cos, ref):
    return cos.view(np.uint32).astype(np.int64) - int(np.asarray(ref, F32).view(np.uint32))


@functools.lru_cache(maxsize=None)
def _bounce_ref(rts, tex_dir):
    s = _oracle_scene(rts, tex_dir)
    objs = sc.scene_objects()
    rng = np.random.default_rng(99)
    crit = critical_cosine()
    total = len(objs) * sc.RAYS_PER_OBJECT
    perm = np.random.default_rng(100).permutation(total)             # the objects, and with them the materials, mixed inside every wave
    where = np.argsort(perm)                                         # ray g of the object order is case where[g]
    seed, warm = sc.bounce_seeds(total)
    I, O, D, T = [], [], [], []
    for k, ob in enumerate(objs):
        o, d, t = sc.object_rays(ob, rng)
        if ob["mat"] == 4 and ob["extra"] == 1.5:
            # front-face rays whose reflectance meets the uniform number of their case, in place of the object's rays 128 ..
            case = where[k * sc.RAYS_PER_OBJECT + 128 + np.arange(sc.SCHLICK_RAYS)]
            o[128:128 + sc.SCHLICK_RAYS], d[128:128 + sc.SCHLICK_RAYS], t[128:128 + sc.SCHLICK_RAYS] = schlick_rays(s, k, ob, rng, seed[case], warm[case])
            # rays whose computed cosine is within 4 ulps of the critical one, up to 64 on either side, in place of the first of the object's
            co, cd, ct = sc.critical_candidates(ob, rng)
            cos, front = glass_cosine(s, np.full(len(co), k, np.int32), co, cd, ct)
            near = ulps_from(cos, crit)
            keep = np.concatenate([np.flatnonzero(~front & (near <= 0) & (near >= -4))[:64], np.flatnonzero(~front & (near > 0) & (near <= 4))[:64]])
            o[:len(keep)], d[:len(keep)], t[:len(keep)] = co[keep], cd[keep], ct[keep]
        I.append(np.full(len(o), k, np.int32)); O.append(o); D.append(d); T.append(t)
    idx, o, d, t = np.concatenate(I), np.concatenate(O), np.concatenate(D), np.concatenate(T)
    assert len(idx) == total
    idx, o, d, t = idx[perm], o[perm], d[perm], t[perm]
    atten = sc.bounce_attens(len(idx))
    branch, o2, d2, a2, nxt = s.kat_bounce(idx, o, d, t, atten, seed, warm)
    return {"idx": idx, "o": o, "d": d, "t": t, "atten": atten, "seed": seed, "warm": warm, "branch": branch, "o2": o2, "d2": d2, "a2": a2, "next": nxt}


def bounce_preconditions(tmp_path_factory):
    s = oracle_scene(tmp_path_factory)
    r = _bounce_ref(*files(tmp_path_factory))
    objs = sc.scene_objects()
    assert len(r["idx"]) == len(objs) * sc.RAYS_PER_OBJECT
    counts = np.bincount(r["branch"], minlength=10)
    print("bounce: %d rays; per branch %s" % (len(r["idx"]), dict(zip(BR, counts.tolist()))))
    assert len(counts) == 10 and (counts >= 64).all(), counts
    assert counts[BR["glossy_metal"]] >= 64 and counts[BR["glossy_diffuse"]] >= 64          # like_metal decided on both sides of 0.8
    mat = np.array([ob["mat"] for ob in objs])[r["idx"]]
    glass = np.flatnonzero((mat == 4) & (np.array([ob["extra"] for ob in objs])[r["idx"]] == 1.5))
    raw, front = glass_cosine(s, r["idx"][glass], r["o"][glass], r["d"][glass], r["t"][glass])
    near = np.abs(ulps_from(np.minimum(raw, F32(1)), critical_cosine())) <= 4
    br = r["branch"][glass]
    n_cannot, n_refract = int((near & ~front & (br == BR["glass_cannot"])).sum()), int((near & ~front & (br == BR["glass_refract"])).sum())
    all_glass = np.flatnonzero(mat == 4)
    raw_all, front_all = glass_cosine(s, r["idx"][all_glass], r["o"][all_glass], r["d"][all_glass], r["t"][all_glass])
    clamped = int((~front_all & (raw_all > 1)).sum())
    print("bounce: within 4 ulps of the critical cosine %d cannot refract, %d refract; the clamp at 1 acts on %d back-face glass rays" % (n_cannot, n_refract, clamped))
    assert n_cannot >= 1 and n_refract >= 1 and clamped >= 1
    # the reflectance within 2 ulps of the uniform number it is compared with, on both outcomes (where an ulp in the fifth power decides)
    refl = reflectance(np.minimum(raw, F32(1)), FRONT_RATIO)
    close = front & (np.abs(ulps_from(refl, 0) - ulps_from(glass_uniform(r["seed"][glass], r["warm"][glass]), 0)) <= 2)
    n_schlick, n_through = int((close & (br == BR["glass_schlick"])).sum()), int((close & (br == BR["glass_refract"])).sum())
    print("bounce: reflectance within 2 ulps of its uniform number: %d reflect, %d refract" % (n_schlick, n_through))
    assert n_schlick >= 8 and n_through >= 8
    # both faces, grazing incidence and the whole range of lengths are there
    raw_any, front_any = glass_cosine(s, r["idx"], r["o"], r["d"], r["t"])
    length = np.sqrt((r["d"].astype(np.float64) ** 2).sum(axis=1))
    assert front_any.sum() > len(front_any) // 4 and (~front_any).sum() > len(front_any) // 4
    assert (np.abs(raw_any) < 2e-4).sum() >= 64 and length.min() < 2e-3 and length.max() > 5e2
    # every variant of the triangles, and glass with a roughness texture (where the textured roughness must not become ir)
    assert {ob.get("variant") for ob in objs if ob["type"] == 2} == set(range(8))
    assert any(ob["mat"] == 4 and ob["type"] == 2 and ob["rtex"] != "no" for ob in objs)
    return counts, n_cannot, n_refract, clamped


def check_bounce(impl, tmp_path_factory):
    bounce_preconditions(tmp_path_factory)
    r = _bounce_ref(*files(tmp_path_factory))
    alive, o2, d2, a2, nxt = impl.bounce(r["idx"], r["o"], r["d"], r["t"], r["atten"], r["seed"], r["warm"])
    want_alive = (r["branch"] != BR["emissive"]).astype(np.int32)
    inputs = {"object": r["idx"], "o": r["o"], "d": r["d"], "t": r["t"], "atten": r["atten"], "seed": r["seed"], "warm": r["warm"], "oracle's branch": r["branch"]}
    out = {}
    for f, form in enumerate(("shade_hit", "split")):
        out.update({form + " alive": (alive[f], want_alive), form + " origin": (o2[f], r["o2"]), form + " direction": (d2[f], r["d2"]),
                    form + " attenuation": (a2[f], r["a2"]), form + " next": (nxt[f], r["next"])})
    compare(impl.name + " kat_bounce", inputs, out)


# ------------------------------------------------------------------ background
@functools.lru_cache(maxsize=None)
def _miss_ref(rts, tex_dir):
    s = _oracle_scene(rts, tex_dir)
    d, atten = sc.miss_directions()
    return d, atten, {bt: s.kat_miss(d, atten, bt, sc.MISS_BGINT) for bt in range(-1, len(sc.TEXTURES))}


def check_miss(impl, tmp_path_factory):
    d, atten, want = _miss_ref(*files(tmp_path_factory))
    assert len(d) >= sc.MISS_RANDOM + 11 + 128 + sc.MISS_AIMED // 2 and (d == np.array([0, 0, -1], F32)).all(axis=1).any()
    for bt, ref in want.items():
        assert np.isfinite(ref).all()
        compare("%s kat_miss backtex %d" % (impl.name, bt), {"d": d, "atten": atten}, {"rgb": (impl.miss(d, atten, bt, sc.MISS_BGINT), ref)})


# ------------------------------------------------------------------ camera
@functools.lru_cache(maxsize=None)
def camera_ref():
    out = []
    for name, st in sc.camera_views().items():
        x, y, s = sc.camera_pixels(st)
        for seed in sc.CAMERA_SEEDS:
            for stride in sc.camera_strides(st):
                out.append((name, st, seed, stride, x, y, s) + orc().kat_camera(st, sc.CAMERA_W, sc.CAMERA_H, seed, stride, x, y, s))
    return out


def check_camera(impl):
    ref = camera_ref()
    assert len(ref) == 3 * 3 * 2
    wraps = sum(int(((x.astype(np.int64) + y.astype(np.int64) * stride) >= 2 ** 32).sum()) for _, _, _, stride, x, y, _, _, _, _ in ref)
    lens = {name: float(np.abs(o - st[:3]).max()) for name, st, _, _, _, _, _, o, _, _ in ref}
    print("camera: %d pixel seeds wrap 32 bits; largest lens offset per view %s" % (wraps, lens))
    assert wraps >= 100 and lens["lens radius 0"] == 0.0 and lens["lens radius 0.3"] > 0.1
    for name, st, seed, stride, x, y, s, o, d, nxt in ref:
        go, gd, gn = impl.camera(st, sc.CAMERA_W, sc.CAMERA_H, seed, stride, x, y, s)
        out = {}
        for f, form in enumerate(("camera_ray", "split")):
            out.update({form + " origin": (go[f], o), form + " direction": (gd[f], d), form + " next": (gn[f], nxt)})
        compare("%s kat_camera %s, frame seed %d, stride %d" % (impl.name, name, seed, stride), {"x": x, "y": y, "sample": s}, out)


# ------------------------------------------------------------------ store
@functools.lru_cache(maxsize=None)
def store_ref():
    c = sc.store_colours()
    return c, {spp: orc().kat_store(c, spp) for spp in sc.STORE_SPP}


def check_store(impl):
    c, want = store_ref()
    for spp, ref in want.items():
        # the conversion saturates at both ends and maps NaN to 0 somewhere in the set
        assert (ref == 2147483647).any() and (ref == -2147483648).any() and (ref[np.isnan(c)] == 0).all() and np.isnan(c).any()
        assert ((ref > 2 ** 30) & (ref < 2147483647)).any()          # and the largest products below 2^31 are there
        compare("%s kat_store spp %d" % (impl.name, spp), {"colour": c}, {"stored": (impl.store(c, spp), ref)})
