"""What tests/test_trace_host.py and tests/test_gpu_trace.py share beside tests/ray_cases.py and tests/ray_checks.py: the adversarial tmax sets of a
(scene, class) pair, formed from the oracle's own t, and the post-filter they are judged by."""
import numpy as np

import ray_cases as rc

F = np.float32


def tmax_sets(stem, cls, rt):
    """[(name, tmax float32[n])] for the rays of the pair whose oracle t is rt: for a ray the oracle hits, its exact t, the float below, the float
    above, and one of t / 2, 2 t, 0, -1, NaN, +inf; for a ray it misses a random positive value in the first three sets and one of that, 0, -1, NaN, +inf
    in the last.  Four sets of n values: of the rays the oracle hits, a quarter of all values land on the bits of t and a quarter one ulp below."""
    rng = np.random.default_rng(rc.seed_of(stem, cls) + [77])
    n = len(rt)
    rt = np.asarray(rt, F)
    hit = rt > 0
    pos = lambda: np.exp(rng.uniform(np.log(1e-3), np.log(2e4), n)).astype(F)
    safe = np.where(hit, rt, F(1))
    with np.errstate(all="ignore"):
        exact = np.where(hit, safe, pos()).astype(F)
        below = np.where(hit, np.nextafter(safe, F(0)), pos()).astype(F)
        above = np.where(hit, np.nextafter(safe, F(np.inf)), pos()).astype(F)
        pick = rng.integers(0, 6, n)
        table = np.stack([safe / F(2), safe * F(2), np.zeros(n, F), np.full(n, -1, F), np.full(n, np.nan, F), np.full(n, np.inf, F)]).astype(F)
        mixed = table[pick, np.arange(n)]
        mixed = np.where(~hit & (pick < 2), pos(), mixed).astype(F)
    return [("exact", exact), ("below", below), ("above", above), ("mixed", mixed)]


def post_filter(rt, ri, tmax):
    """the oracle's hit (rt, ri: kat_hit's, index 0 on a miss) if its t <= tmax, else a miss, in dr_trace_rays' convention: (t, -1 on a miss; object,
    -1 on a miss; occluded)"""
    rt = np.asarray(rt, F)
    with np.errstate(invalid="ignore"):
        keep = (rt > 0) & (rt <= (np.asarray(tmax, F) if tmax is not None else F(np.inf)))
    return np.where(keep, rt, F(-1)).astype(F), np.where(keep, ri, -1).astype(np.int32), keep.astype(np.int32)
