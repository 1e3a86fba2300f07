"""A numpy restatement of adaptive sampling (include/dogeray_amd.h "adaptive sampling", dogeray_amd/csrc/device_adaptive.hpp), independent of the
source under test: the selection over whole planes at once (int64 / uint64 / float64, float32 for sigma and its comparison -- the arithmetic of
tests/moments_checks.py) and the fold under a tile mask (the split of a tile order: tests/split_cases.py).  Shared by
tests/test_adaptive_host.py and tests/test_gpu_adaptive.py.  Planes are indexed [x, y] like dr_accum_read."""
import numpy as np

import moments_checks as mc

DEFAULTS = {"tolerance": 1.0, "min_samples": 4, "max_samples": 0, "tile_pixels": 1}


def grid(settings13, W, H):
    """(gx, gy): the 8x8 tiles of the view's pixel grid"""
    div = int(settings13[11])
    return W // div // 8, H // div // 8


def samples(hist, gx, gy, divide_by):
    """n = hist + divide_by over the grid, int64[8 gx, 8 gy]"""
    h = np.zeros((8 * gx, 8 * gy), np.int64) if hist is None else np.asarray(hist)[:8 * gx, :8 * gy].astype(np.int64)
    return h + int(divide_by)


def sigma(acc, hist, m2, gx, gy, divide_by):
    """(estimated, sigma float32) over the grid: dr_accum_error's estimate"""
    n = samples(hist, gx, gy, divide_by)
    est, var = mc.variance(np.asarray(acc, np.int32)[:8 * gx, :8 * gy], np.asarray(m2, np.uint64)[:8 * gx, :8 * gy], n)
    return est, np.where(est, np.sqrt(var), 0.0).astype(np.float32)


def asks(acc, hist, m2, gx, gy, divide_by, **params):
    """bool[8 gx, 8 gy]: the pixels that ask, and the two reasons apart (few: n < min_samples; noisy: the estimate above the tolerance, under the cap)"""
    p = dict(DEFAULTS, **params)
    n = samples(hist, gx, gy, divide_by)
    est, sig = sigma(acc, hist, m2, gx, gy, divide_by)
    few = n < p["min_samples"]
    under = np.ones_like(few) if p["max_samples"] == 0 else n < p["max_samples"]
    noisy = under & est & (sig > np.float32(p["tolerance"]))
    return few | noisy, few, noisy


def tiles_of(pixels, gx, gy):
    """a plane over the grid [8 gx, 8 gy] as [gx * gy, 64]: tile t = col * gy + by, lane l = pixel (8 col + (l >> 3), 8 by + (l & 7))"""
    return pixels.reshape(gx, 8, gy, 8).transpose(0, 2, 1, 3).reshape(gx * gy, 64)


def select(acc, hist, m2, gx, gy, divide_by, **params):
    """(flags uint8[gx * gy], dict tiles, active_tiles, pixels, asking_pixels)"""
    p = dict(DEFAULTS, **params)
    a, _, _ = asks(acc, hist, m2, gx, gy, divide_by, **params)
    per_tile = tiles_of(a, gx, gy).sum(axis=1)
    flags = (per_tile >= p["tile_pixels"]).astype(np.uint8)
    return flags, {"tiles": gx * gy, "active_tiles": int(flags.sum()), "pixels": 64 * gx * gy, "asking_pixels": int(a.sum())}


def tile_max_sigma(acc, hist, m2, gx, gy, divide_by):
    """float32[gx * gy]: the largest sigma of each tile"""
    return tiles_of(sigma(acc, hist, m2, gx, gy, divide_by)[1], gx, gy).max(axis=1)


def pixel_mask(flags, gx, gy, W, H):
    """bool[W, H]: the pixels of the flagged tiles"""
    m = np.zeros((W, H), bool)
    m[:8 * gx, :8 * gy] = np.repeat(np.repeat(np.asarray(flags, bool).reshape(gx, gy), 8, axis=0), 8, axis=1)
    return m


def fold(acc, hist, m2, frames, flags, gx, gy):
    """(acc, hist, m2) after the frames (int32[n, W, H, 3]) are folded into the pixels of the flagged tiles: wrapping sums, saturating M2,
    hist += n there; every other pixel as it was.  hist None: zeros."""
    acc = np.asarray(acc, np.int32)
    W, H = acc.shape[0], acc.shape[1]
    hist = np.zeros((W, H), np.int32) if hist is None else np.asarray(hist, np.int32)
    m = pixel_mask(flags, gx, gy, W, H)
    a, s = acc.astype(np.int64), np.asarray(m2, np.uint64).copy()
    for f in frames:
        a = a + np.asarray(f, np.int64)
        s = mc.sat_add(s, mc.square(f))
    a = ((a + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)
    h = ((hist.astype(np.int64) + len(frames) + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int32)
    return np.where(m[..., None], a, acc), np.where(m, h, hist), np.where(m, s, np.asarray(m2, np.uint64))
