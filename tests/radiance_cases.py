"""What tests/test_radiance_host.py and tests/test_gpu_radiance.py share: the rays aimed at the all-materials scene of tests/shade_cases.py, their
seeds and skips, and the reference -- raycolor's loop composed in Python from the oracle's functions alone (kat_hit, kat_bounce, kat_miss), the
generator's position after every bounce found in the oracle's own sequence of outputs (kat_rng_u32).  Deterministic; nothing here looks at what the
product computes."""
import functools

import numpy as np

import shade_cases as sc

F32 = np.float32
GOLDEN_RATIO = sc.GOLDEN_RATIO
M_WORDS = 4096                 # generator outputs per path within which its position must be found (raise it if a path draws more; never lower it per case)
N_AIMED, N_SKY = 2000, 200
SPPS = (1, 3)
DEPTHS = (1, 2, 10)
BACKGROUNDS = (-1, sc.TEX_TWO)
BGINT = 0.75
EMISSIVE = 9                   # orc.BRANCHES' last: the path ends with the attenuation output as its radiance


def shading_rays(n_aimed=N_AIMED, n_sky=N_SKY):
    """(o, d) float32 [n_aimed + n_sky, 3]: rays from points on a sphere around the scene towards points on its objects (ray k at object k % 70,
    directions of every length between 1e-2 and 1e2), then rays from the same sphere straight away from the scene, at the sky"""
    objs = sc.scene_objects()
    rng = np.random.default_rng(20241020)
    centre = np.array([4.0 * (len(objs) - 1) / 2.0, 0.0, 0.0])      # the objects stand at x = 0, 4, .. 4 (n - 1)
    radius = centre[0] + 20.0
    n = n_aimed + n_sky
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    origin = centre + radius * u
    target = np.empty((n_aimed, 3))
    for k, ob in enumerate(objs):
        sel = np.arange(k, n_aimed, len(objs))
        target[sel] = sc._surface_points(ob, rng, len(sel))[0]
    d = np.concatenate([target - origin[:n_aimed], u[n_aimed:]])
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * 10.0 ** rng.uniform(-2, 2, (n, 1))
    return np.ascontiguousarray(origin, F32), np.ascontiguousarray(d, F32)


def shading_seeds(n, skipped):
    """(base seed, seeds or None, skip or None): without skips the rays take base seed + i, with them seeds of their own and 0 .. 7 outputs discarded"""
    if not skipped:
        return 12345, None, None
    rng = np.random.default_rng(77)
    return 0, rng.integers(0, 2 ** 64, n, dtype=np.uint64), rng.integers(0, 8, n).astype(np.int32)


def oracle_scene(rts, tex):
    """an oracle scene of the caller's own (tests/shade_checks.py keeps its own unchanged), its tree built for kat_hit"""
    from oracle import orc
    s = orc.Scene(rts, tex)
    s.build_bvh()
    return s


@functools.lru_cache(maxsize=8)
def _words(seed_bytes):
    from oracle import orc
    seeds = np.frombuffer(seed_bytes, np.uint64)
    return np.stack([orc.kat_rng_u32(int(s), M_WORDS) for s in seeds])


def position_after(words, pair, at_least):
    """where in each row of words (the generator's outputs) the two outputs `pair` stand, at or after the position at_least: the generator's position
    after the draws of a bounce.  A pair that is not found fails the test."""
    k = np.arange(M_WORDS - 1)[None]
    match = (words[:, :-1] == pair[:, :1]) & (words[:, 1:] == pair[:, 1:]) & (k >= at_least[:, None])
    assert match.any(axis=1).all(), "the generator's position was not found within %d outputs" % M_WORDS
    return match.argmax(axis=1).astype(np.int32)


def oracle_radiance(scene, o, d, spp, max_depth, bgint, backtex, seed=0, seeds=None, skip=None):
    """dr_trace_radiance's contract on the oracle: per ray the float32 sum, in sample order from 0, of raycolor's loop -- kat_hit; t > 0: kat_bounce (an
    emissive branch ends the path with its radiance), else kat_miss ends it; a path that is still alive after max_depth bounces ends with 0 --, and
    the kat_hit calls.  Also the bounces per branch, the paths that ended with their depth exhausted and the first rays that missed."""
    n = len(o)
    S = np.asarray(seeds, np.uint64) if seeds is not None else (np.arange(n, dtype=np.uint64) + np.uint64(seed % 2 ** 64))
    total, bounces = np.zeros((n, 3), F32), np.zeros(n, np.int32)
    branches, exhausted, first_miss = np.zeros(10, np.int64), 0, 0
    with np.errstate(over="ignore"):
        for s in range(spp):
            ss = S + np.uint64((s * GOLDEN_RATIO) % 2 ** 64)
            words = _words(ss.tobytes())
            ro, rd, at = np.array(o, F32), np.array(d, F32), np.ones((n, 3), F32)
            warm = np.zeros(n, np.int32) if skip is None else np.array(skip, np.int32)
            result = np.zeros((n, 3), F32)
            alive = np.arange(n)
            for depth in range(max_depth):
                if len(alive) == 0:
                    break
                t, idx = scene.kat_hit(ro[alive], rd[alive])
                bounces[alive] += 1
                hit = t > 0
                if depth == 0:
                    first_miss += int((~hit).sum())
                gone = alive[~hit]
                if len(gone):
                    result[gone] = scene.kat_miss(rd[gone], at[gone], backtex, bgint)
                on = alive[hit]
                if len(on) == 0:
                    alive = on
                    break
                br, o2, d2, a2, nx = scene.kat_bounce(idx[hit], ro[on], rd[on], t[hit], at[on], ss[on], warm[on])
                branches += np.bincount(br, minlength=10)
                ended = br == EMISSIVE
                result[on[ended]] = a2[ended]
                alive = on[~ended]
                ro[alive], rd[alive], at[alive] = o2[~ended], d2[~ended], a2[~ended]
                warm[alive] = position_after(words[alive], nx[~ended], warm[alive])
            exhausted += len(alive)
            total = total + result
    return {"radiance": total, "bounces": bounces, "branches": branches, "exhausted": exhausted, "first_miss": first_miss}
