"""The inputs of the shading step's known-answer tests (tests/test_shade_host.py, tests/test_gpu_shade.py): generator states for the rejection samplers,
squared lengths around 1, texture coordinates at the wrap and clamp edges, one generated scene with every material on triangles and spheres and the rays
that bounce off it, background directions, camera pixels and colours to store.  Deterministic: every random number comes from a seeded numpy generator.
Nothing here looks at a result; tests/shade_checks.py runs the oracle on these inputs, asserts that they reach the branches they are made for, and compares."""
import os

import numpy as np

F32 = np.float32
GOLDEN_RATIO = 0x9E3779B97F4A7C15
CORNER_SEEDS = (0, 1, 12345, 2 ** 32 + 7, 2 ** 64 - 1, 1 + 1000003 * 5 + 255 + 255 * 256)      # test_gpu_parity.py test_rng_xorwow's


def f32_neighbours(v):
    """float32 v, the float below it and the float above it"""
    v = F32(v)
    return [np.nextafter(v, F32(-np.inf)), v, np.nextafter(v, F32(np.inf))]


# ------------------------------------------------------------------ samplers
SAMPLER_N = 1 << 20
SAMPLER_KINDS = (0, 2, 3, 3)


def searched_states():
    """the states of tests/golden/shade_sampler_seeds.json (make_shade_seeds.py: found by a search, what the seed formula reaches too rarely)"""
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shade_sampler_seeds.json")) as f:
        st = json.load(f)["states"]
    return np.array([s["seed"] for s in st], np.uint64), np.array([s["warm"] for s in st], np.int32), np.array([s["kind"] for s in st], np.int32)


def sampler_states():
    """(seed uint64[n], warm int32[n], kind int32[n]): 2^20 states whose kinds mix inside every wave of 64, then the corner seeds with every kind, then
    the searched states"""
    i = np.arange(SAMPLER_N, dtype=np.uint64)
    seed = i * np.uint64(GOLDEN_RATIO) + np.uint64(12345)          # (mod 2^64)
    warm = (i % np.uint64(7)).astype(np.int32)
    kind = np.array(SAMPLER_KINDS, np.int32)[(i % np.uint64(4)).astype(np.int64)]
    cs, cw, ck = [], [], []
    for s in CORNER_SEEDS:
        for w in (0, 5):
            for k in (3, 2, 0):
                cs.append(s); cw.append(w); ck.append(k)
    ss, sw, sk = searched_states()
    return (np.concatenate([seed, np.array(cs, np.uint64), ss]), np.concatenate([warm, np.array(cw, np.int32), sw]),
            np.concatenate([kind, np.array(ck, np.int32), sk]))


# ------------------------------------------------------------------ outside_unit
def outside_values():
    """every float within 2^18 ulps of 1.0, both sides (524 289 values), and the specials"""
    bits = (np.int64(0x3f800000) + np.arange(-(1 << 18), (1 << 18) + 1, dtype=np.int64)).astype(np.uint32)
    one = F32(1.0)
    special = np.array([0.0, -0.0, 3.0, np.nextafter(one, F32(0)), np.nextafter(one, F32(2)), np.inf, np.nan], F32)
    return np.concatenate([bits.view(F32), special])


# ------------------------------------------------------------------ the scene: textures and objects
# (file name, width, height, scenegen's pattern; None: the committed tests/golden/textures/a.ppm, 64 x 64) -- in the sorted order a scene numbers them
TEXTURES = (("a.ppm", 64, 64, None), ("synth_albedo.ppm", 128, 128, 0), ("synth_rough.ppm", 64, 64, 1), ("testtwo.ppm", 96, 64, 0))
TEX_A, TEX_ALBEDO, TEX_ROUGH, TEX_TWO = 0, 1, 2, 3
MATERIALS = (0, 1, 2, 3, 4, 5, 7)
# what a triangle varies in besides material and add_x
VARIANTS = ("face normal from the edges", "face normal given", "smooth, vertex normals", "smooth flag, n1.z sentinel", "checker", "albedo texture",
            "roughness texture", "both textures, texture coordinates outside [0, 1] and negative")


def scene_objects():
    """The objects of the generated scene as dicts (type 2: triangle, 0: sphere): every material x add_x on spheres (14) and on triangles in four of the
    eight VARIANTS each (56).  Glass has ir 1.0 with add_x 0 and 1.5 with add_x 1; every other material carries 0.3 there (its roughness)."""
    rng = np.random.default_rng(20240607)
    objs = []
    combo = 0
    for mat in MATERIALS:
        for add_x in (0, 1):
            extra = (1.5 if add_x else 1.0) if mat == 4 else 0.3
            col = [round(float(v), 3) for v in rng.uniform(0.2, 0.95, 3)]
            c = [4.0 * len(objs), round(float(rng.uniform(-1, 1)), 3), round(float(rng.uniform(-1, 1)), 3)]
            objs.append({"type": 0, "pos": c, "radius": round(float(rng.uniform(0.4, 1.2)), 3), "col": col, "extra": extra, "add_x": add_x, "mat": mat})
            for variant in (combo % 8, (combo + 3) % 8, (combo + 5) % 8, (combo + 6) % 8):
                v0 = np.array([4.0 * len(objs), rng.uniform(-1, 1), rng.uniform(-1, 1)]).round(3)
                v1 = (v0 + np.array([rng.uniform(0.8, 1.6), rng.uniform(-0.4, 0.4), rng.uniform(-0.4, 0.4)])).round(3)
                v2 = (v0 + np.array([rng.uniform(-0.4, 0.4), rng.uniform(0.8, 1.6), rng.uniform(-0.5, 0.5)])).round(3)
                fn = np.cross(v1 - v0, v2 - v0)
                fn = fn / np.linalg.norm(fn)
                o = {"type": 2, "v0": v0.tolist(), "v1": v1.tolist(), "v2": v2.tolist(), "col": [round(float(v), 3) for v in rng.uniform(0.2, 0.95, 3)],
                     "extra": extra, "add_x": add_x, "mat": mat, "variant": variant, "norm": None, "vn": None, "smooth": 0, "checker": 0, "tex": "no", "rtex": "no",
                     "tc": None}
                tilt = [(fn + rng.uniform(-0.3, 0.3, 3)).round(4).tolist() for _ in range(3)]
                if variant >= 1:
                    o["norm"] = (fn * 1.7).round(4).tolist()          # (not of unit length: getnormal normalises it)
                if variant == 2:
                    o["smooth"], o["vn"] = 1, tilt
                if variant == 3:
                    o["smooth"] = 1                                  # n1 .. n3 stay the file's defaults: n1.z is the -20 sentinel
                if variant == 4:
                    o["checker"] = 1
                if variant in (5, 7):
                    o["tex"] = "synth_albedo" if variant == 5 else "testtwo"
                if variant in (6, 7):
                    o["rtex"] = "synth_rough"
                if variant == 7:
                    o["tc"] = [[-1.3, 2.2], [0.4, -0.7], [3.1, 0.5]]
                objs.append(o)
            combo += 1
    return objs


def rts_text(objs):
    """The .rts file of the objects (38 columns a line, the column order of the reader)"""
    def num(v):
        return repr(float(v))
    lines = []
    for o in objs:
        if o["type"] == 0:
            f = [num(v) for v in o["pos"]] + ["0"] + [num(v) for v in o["col"]] + [num(o["extra"]), num(o["add_x"]), num(o["radius"]), "0", "0", str(o["mat"])]
            lines.append(",".join(f))
            continue
        norm = o["norm"] or [-2, -3, -20]
        vn = o["vn"] or [[-2, -3, -20]] * 3
        tc = o["tc"] or [[0, 1], [0, 0], [1, 0]]
        f = ([num(v) for v in o["v0"]] + ["2"] + [num(v) for v in o["col"]] + [num(o["extra"]), num(o["add_x"])] + [num(v) for v in o["v1"]] + [str(o["mat"])] +
             [num(v) for v in o["v2"]] + [num(v) for v in norm] + [num(v) for n in vn for v in n] + [num(v) for t in tc for v in t] +
             [str(o["smooth"]), str(o["checker"]), o["tex"], o["rtex"]])
        assert len(f) == 38
        lines.append(",".join(f))
    return "\n".join(lines) + "\n"


# ------------------------------------------------------------------ texel fetch
TEX_RANDOM = 100_000


def tex_axis_values(size):
    """The coordinates for an axis of `size` texels: k / size and its float neighbours for k in {0, 1, size / 2, size - 1, size}; the same shifted by -1, -2
    and +3; and the specials"""
    base = []
    for k in (0, 1, size // 2, size - 1, size):
        base += f32_neighbours(F32(k) / F32(size))
    base = np.array(base, F32)
    vals = [base] + [base + F32(s) for s in (-1.0, -2.0, 3.0)]
    special = np.array([-0.0, 1.0 - 2.0 ** -24, 2.0 ** 23 + 0.5, -2.0 ** 23 - 0.5, 1e30, -1e30, np.inf, -np.inf, np.nan], F32)
    return np.concatenate(vals + [special])


def tex_cases():
    """(tex int32[n], u float32[n], v float32[n]): per texture the cross product of its axes' values (u and v independently), then 10^5 uniform pairs"""
    rng = np.random.default_rng(7)
    T, U, V = [], [], []
    for t, (_, w, h, _) in enumerate(TEXTURES):
        uu, vv = np.meshgrid(tex_axis_values(w), tex_axis_values(h), indexing="ij")
        U.append(uu.ravel()); V.append(vv.ravel())
        U.append(rng.uniform(-3, 3, TEX_RANDOM).astype(F32)); V.append(rng.uniform(-3, 3, TEX_RANDOM).astype(F32))
        T.append(np.full(uu.size + TEX_RANDOM, t, np.int32))
    return np.concatenate(T), np.concatenate(U), np.concatenate(V)


# ------------------------------------------------------------------ one bounce
RAYS_PER_OBJECT = 512
CRITICAL_CANDIDATES = 4096


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _frame(n):
    """two unit vectors orthogonal to each n (float64 [m, 3])"""
    a = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    t1 = _unit(np.cross(n, a))
    return t1, np.cross(n, t1)


def _surface_points(o, rng, m):
    """m points inside object o and the geometric unit normal there (float64)"""
    if o["type"] == 0:
        n = _unit(rng.normal(size=(m, 3)))
        return np.array(o["pos"]) + o["radius"] * n, n
    v0, v1, v2 = (np.array(o[k]) for k in ("v0", "v1", "v2"))
    a = rng.uniform(0.05, 0.9, m)
    b = rng.uniform(0.05, 0.9, m) * (0.95 - a)
    n = _unit(np.cross(v1 - v0, v2 - v0))
    return v0 + a[:, None] * (v1 - v0) + b[:, None] * (v2 - v0), np.broadcast_to(n, (m, 3)).copy()


def rays_at(p, n, cos, back, phi, L, s):
    """The rays that reach the points p under the cosine `cos` to the normal n from its front (against n) or its back, at azimuth phi: the direction has
    length L, the origin lies s unit lengths before p and t = s / L (float32 origin, direction, t)"""
    t1, t2 = _frame(n)
    sin = np.sqrt(np.maximum(0.0, 1.0 - cos * cos))
    side = np.where(back, 1.0, -1.0)
    du = side[:, None] * cos[:, None] * n + sin[:, None] * (np.cos(phi)[:, None] * t1 + np.sin(phi)[:, None] * t2)
    return (p - du * s[:, None]).astype(F32), (du * L[:, None]).astype(F32), (s / L).astype(F32)


def _rays(p, n, cos, back, rng, length=None):
    """rays_at with random azimuths, lengths of 1e-3 .. 1e3 (log-uniform) and origins 0.5 .. 5 unit lengths away"""
    m = len(p)
    phi = rng.uniform(0, 2 * np.pi, m)
    L = 10.0 ** rng.uniform(-3, 3, m) if length is None else length
    return rays_at(p, n, cos, back, phi, L, rng.uniform(0.5, 5.0, m))


SCHLICK_RAYS = 96


def schlick_frames(o, rng, m=SCHLICK_RAYS):
    """what rays_at needs besides the cosine, for m front-face rays of a glass object: tests/shade_checks.py bisects the cosine of each until its
    reflectance meets the uniform number it will be compared with"""
    p, n = _surface_points(o, rng, m)
    return p, n, np.zeros(m, bool), rng.uniform(0, 2 * np.pi, m), 10.0 ** rng.uniform(-1, 1, m), rng.uniform(0.5, 5.0, m)


def object_rays(o, rng, m=RAYS_PER_OBJECT):
    """m rays for one object: three quarters with the incidence from normal to grazing (cos 1 .. 1e-4, log-spaced) on alternating faces, an eighth exactly
    along the normal onto each face (where the computed cosine can round above 1)"""
    g = m * 3 // 4
    p, n = _surface_points(o, rng, m)
    cos = np.concatenate([10.0 ** np.linspace(0, -4, g), np.ones(m - g)])
    back = np.arange(m) % 2 == 1
    return _rays(p, n, cos, back, rng)


def critical_candidates(o, rng, m=CRITICAL_CANDIDATES):
    """Back-face rays for a glass object of ir 1.5 whose cosine lies within a few 1e-6 of the critical one (sqrt(1 - 1 / 1.5^2)): tests/shade_checks.py
    keeps the ones whose COMPUTED cosine is within 4 ulps of the float at which 'cannot refract' flips"""
    p, n = _surface_points(o, rng, m)
    cos = np.sqrt(1.0 - 1.0 / 2.25) * (1.0 + rng.uniform(-1.5e-6, 1.5e-6, m))
    return _rays(p, n, cos, np.ones(m, bool), rng, length=10.0 ** rng.uniform(-1, 1, m))


def bounce_seeds(n):
    i = np.arange(n, dtype=np.uint64)
    return i * np.uint64(GOLDEN_RATIO) + np.uint64(777), (i % np.uint64(5)).astype(np.int32)


def bounce_attens(n):
    a = np.random.default_rng(11).uniform(0.05, 1.0, (n, 3)).astype(F32)
    a[::7] = 1.0
    return a


# ------------------------------------------------------------------ background
MISS_RANDOM = 10_000
MISS_AIMED = 2_000
MISS_BGINT = 0.75


def miss_directions():
    """10^4 random directions; (0, 0, -1) -- the environment lookup divides by m = 0 there -- and the same with a last-bit x; the six axes; lengths 1e-20
    and 1e20; and directions aimed at the texel boundaries of the environment lookup (tt.x = k / 128 up to rounding), where an ulp in m moves the texel"""
    rng = np.random.default_rng(5)
    d = [_unit(rng.normal(size=(MISS_RANDOM, 3))) * 10.0 ** rng.uniform(-2, 2, (MISS_RANDOM, 1))]
    tiny = float(np.nextafter(F32(0), F32(1)))
    d.append(np.array([[0, 0, -1], [tiny, 0, -1], [-tiny, 0, -1], [2.0 ** -24, 0, -1], [0, tiny, -1],
                       [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64))
    u = _unit(rng.normal(size=(64, 3)))
    d += [u * 1e-20, u * 1e20]
    uz = rng.uniform(-0.9, 0.9, MISS_AIMED)
    k = rng.integers(1, 128, MISS_AIMED)
    ux = (k / 128.0 - 0.5) * 2.0 * np.sqrt(2.0 * (1.0 + uz))
    ok = ux * ux + uz * uz < 0.999
    ux, uz = ux[ok], uz[ok]
    uy = np.sqrt(1.0 - ux * ux - uz * uz) * np.where(rng.uniform(size=len(ux)) < 0.5, -1.0, 1.0)
    d.append(np.stack([ux, uy, uz], 1) * 10.0 ** rng.uniform(-1, 1, (len(ux), 1)))
    d = np.concatenate(d).astype(F32)
    atten = rng.uniform(0.05, 1.0, d.shape).astype(F32)
    atten[::5] = 1.0
    return d, atten


# ------------------------------------------------------------------ camera
CAMERA_W, CAMERA_H = 320, 192
CAMERA_SEEDS = (0, 2 ** 32 + 7, 2 ** 64 - 1)
CAMERA_SAMPLES = (0, 3)
CAMERA_WRAP_STRIDE = 0x02000001              # x + y * stride passes 2^32 from y = 128 on
CAMERA_RANDOM = 1000


def camera_views():
    """name -> settings13: campos, look, aperture (twice the lens radius), focus distance, fov, depth, samples, preview divisor, backtex"""
    def st(aperture, div):
        return np.array([7.358891, -6.925791, 4.958309, 0.3, -0.2, 0.1, aperture, 9.5, 45, 5, 4, div, -1], F32)
    return {"lens radius 0": st(0.0, 1), "lens radius 0.3": st(0.6, 1), "preview divisor 4": st(0.01, 4)}


def camera_pixels(settings13):
    """(x, y, sample) of the view's pixel grid: its four corners and 1000 random pixels, samples 0 and 3 of each"""
    div = int(settings13[11])
    gw, gh = CAMERA_W // div // 8 * 8, CAMERA_H // div // 8 * 8
    rng = np.random.default_rng(3)
    x = np.concatenate([[0, gw - 1, 0, gw - 1], rng.integers(0, gw, CAMERA_RANDOM)]).astype(np.int32)
    y = np.concatenate([[0, 0, gh - 1, gh - 1], rng.integers(0, gh, CAMERA_RANDOM)]).astype(np.int32)
    s = np.repeat(np.array(CAMERA_SAMPLES, np.int32), len(x))
    return np.tile(x, 2), np.tile(y, 2), s


def camera_strides(settings13):
    """the launch's own stride (8 * its block columns) and one for which x + y * stride wraps 32 bits"""
    return (8 * (CAMERA_W // int(settings13[11]) // 8), CAMERA_WRAP_STRIDE)


# ------------------------------------------------------------------ store
STORE_SPP = (1, 3)


def store_colours():
    """float32[n, 3]: each special value in every channel beside the others', then random colours"""
    vals = [0.0, -0.0, 1.0, 1e30, -1e30, np.inf, -np.inf, np.nan]
    vals += f32_neighbours(F32(1) / F32(255)) + f32_neighbours(F32(3) / F32(255)) + f32_neighbours(1.0) + f32_neighbours(3.0)
    vals += f32_neighbours(8421504.0) + f32_neighbours(3 * 8421504.0) + f32_neighbours(-8421504.0) + f32_neighbours(-3 * 8421504.0)      # x 255 crosses 2^31
    v = np.array(vals, F32)
    rows = [np.stack([v, np.roll(v, 1), np.roll(v, 5)], 1), np.stack([v, v, v], 1)]
    rows.append(np.random.default_rng(9).uniform(0, 4, (1000, 3)).astype(F32))
    return np.concatenate(rows)


def write_scene(directory, scenegen):
    """Writes the textures (into directory/tex) and the scene; returns (path of the .rts, texture directory)"""
    import subprocess
    tex = os.path.join(directory, "tex")
    os.makedirs(tex, exist_ok=True)
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "textures")
    for name, w, h, pattern in TEXTURES:
        if pattern is None:
            with open(os.path.join(golden, name), "rb") as f, open(os.path.join(tex, name), "wb") as g:
                g.write(f.read())
        else:
            subprocess.check_call([scenegen, "ppm", os.path.join(tex, name), str(w), str(h), str(pattern)])
    path = os.path.join(directory, "shade.rts")
    with open(path, "w") as f:
        f.write(rts_text(scene_objects()))
    return path, tex
