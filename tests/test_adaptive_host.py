"""Adaptive sampling without a GPU: the host build of its device functions (tools/host_kernel/hk_accum.hpp hk_adaptive_select / hk_subset_split /
hk_adaptive_add = device_adaptive.hpp compiled for the CPU) against the numpy restatement (tests/adaptive_checks.py), bit for bit, over the
adversarial planes of tests/plane_cases.py; every edge of the selection is asserted to be reached by a pixel; the split against random flags; the
launch-site rule of launch_state.hpp; the surface (symbols, struct layouts, refusals of the judge)."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import adaptive_checks as ac
import moments_checks as mc
import plane_cases as pc
import split_cases as sp

sys.path.insert(0, os.path.join(ROOT, "tools"))

MAX_REGIONS = 8
# a view of the cube scene's kind; element 11 is the preview divisor
ST = np.array([7.358891, -6.925791, 4.958309, 0.0, 0.0, 0.0, 0.01, 3.0, 45.0, 10.0, 1.0, 1.0, -1.0], np.float32)


def st_div(div):
    st = ST.copy()
    st[11] = div
    return st


# accumulator size, divisor -> tile grid: 141 x 99 -> 17 x 12, with divisor 2 -> 8 x 6 (a grid much smaller than the accumulator), 38 x 11 -> 4 x 1,
# 13 x 9 -> 1 x 1
VIEWS = ((pc.BIG, 1), (pc.BIG, 2), (pc.TAIL2, 1), (pc.TILE, 1))


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


def planes(W, H, name, with_hist):
    acc = pc.make_acc(name, W, H)
    return acc, (pc.hist(W, H) if with_hist else None), pc.m2_wide(W, H, acc)


def check_select(hk, acc, hist, m2, st, divide_by, **params):
    """host build == restatement: flags and counts; returns the restatement's (flags, counts)"""
    W, H = acc.shape[:2]
    gx, gy = ac.grid(st, W, H)
    flags, counts = hk.adaptive_select(acc, hist, m2, st, divide_by, **params)
    want_flags, want = ac.select(acc, hist, m2, gx, gy, divide_by, **params)
    assert (counts["gx"], counts["gy"]) == (gx, gy)
    assert np.array_equal(flags, want_flags), (W, H, divide_by, params, int((flags != want_flags).sum()))
    assert {k: counts[k] for k in want} == want, (W, H, divide_by, params)
    return want_flags, want


def test_grids():
    assert [ac.grid(st_div(d), W, H) for (W, H), d in VIEWS] == [(17, 12), (8, 6), (4, 1), (1, 1)]
    # the tiles' lane mapping, pixel by pixel
    gx, gy = 3, 2
    p = np.arange(24 * 16).reshape(24, 16)
    t = ac.tiles_of(p, gx, gy)
    for tile in range(gx * gy):
        col, by = tile // gy, tile % gy
        for lane in (0, 1, 7, 8, 9, 63):
            assert t[tile, lane] == p[8 * col + (lane >> 3), 8 * by + (lane & 7)]


@pytest.mark.parametrize("view", VIEWS, ids=lambda v: "%dx%d/%d" % (v[0][0], v[0][1], v[1]))
def test_selection_equals_the_restatement(hk, view):
    (W, H), div = view
    st = st_div(div)
    gx, gy = ac.grid(st, W, H)
    ran = 0
    for name in ("wide", "mixed"):
        for with_hist in (False, True):
            acc, hist, m2 = planes(W, H, name, with_hist)
            _, sig = ac.sigma(acc, hist, m2, gx, gy, 16)
            some = float(np.sort(sig.reshape(-1))[int(0.98 * (sig.size - 1))])
            for divide_by in (0, 1, 2, 3, 4, 8, 9, 16):
                for params in ({"tolerance": 0.0}, {"tolerance": 1e9}, {"tolerance": some, "tile_pixels": 2}, {"tolerance": some, "max_samples": 9},
                               {"tolerance": 0.0, "min_samples": 2, "max_samples": 3, "tile_pixels": 64}):
                    check_select(hk, acc, hist, m2, st, divide_by, **params)
                    ran += 1
    assert ran == 160


def test_selection_edges_are_reached(hk):
    """n = 0, 1, min_samples - 1, min_samples, max_samples - 1, max_samples; sigma exactly the tolerance; saturated M2; tile_pixels 1, 2, 64 -- each on
    the planes the equality above runs over (the history plane's zero columns give n = divide_by), each reached by a pixel or a tile"""
    (W, H), st = pc.BIG, st_div(1)
    gx, gy = ac.grid(st, W, H)
    acc, hist, m2 = planes(W, H, "mixed", True)
    zero = np.zeros((8 * gx, 8 * gy), bool)
    zero[::5] = True                                                       # pc.hist's zero columns
    P = {"tolerance": 0.0, "min_samples": 4, "max_samples": 9}
    for divide_by, n_is, few_there, may_be_noisy in ((0, 0, True, False), (1, 1, True, False), (3, 3, True, True), (4, 4, False, True), (8, 8, False, True), (9, 9, False, False)):
        n = ac.samples(hist, gx, gy, divide_by)
        asks, few, noisy = ac.asks(acc, hist, m2, gx, gy, divide_by, **P)
        at = zero & (n == n_is)
        assert at.sum() >= 8 * gy, divide_by
        assert few[at].all() == few_there and few[at].any() == few_there, divide_by
        if few_there:
            assert asks[at].all()                                          # n < min_samples asks whatever the estimate says (n < 2: there is none)
        elif may_be_noisy:
            assert noisy[at].any() and not noisy[at].all()                 # decided by the estimate: noisy pixels and quiet ones (M2 = 0 rows)
            assert np.array_equal(asks[at], noisy[at])
        else:
            assert not asks[at].any()                                      # n >= max_samples: never
        check_select(hk, acc, hist, m2, st, divide_by, **P)
    # without a cap the same pixels at n = 9 are judged by their estimate
    asks, _, noisy = ac.asks(acc, hist, m2, gx, gy, 9, tolerance=0.0)
    assert noisy[zero].any()
    # sigma exactly equal to the tolerance does not ask: the tolerance is one pixel's own float32 sigma
    est, sig = ac.sigma(acc, hist, m2, gx, gy, 16)
    finite = est & np.isfinite(sig) & (sig > 0)
    tol = float(np.sort(sig[finite])[finite.sum() // 2])
    asks, few, noisy = ac.asks(acc, hist, m2, gx, gy, 16, tolerance=tol)
    equal = est & (sig == np.float32(tol))
    assert equal.any() and not few.any() and not asks[equal].any()
    assert asks[est & (sig > np.float32(tol))].all() and (sig > np.float32(tol)).any() and (finite & (sig < np.float32(tol))).any()
    check_select(hk, acc, hist, m2, st, 16, tolerance=tol, tile_pixels=1)
    # saturated M2 (2^64 - 1): estimated, finite, asked about like any other
    sat = np.asarray(m2)[:8 * gx, :8 * gy] == np.uint64(pc.U64_MAX)
    assert (sat & est).any() and np.isfinite(sig[sat & est]).all() and asks[sat & est].any()
    # tile_pixels: tiles with 0, 1, 2 and 64 asking pixels exist, and the flag turns exactly at the threshold
    per_tile = {}
    for tol_q in (0.0, 0.98, 0.995, 0.9995):
        t = 0.0 if tol_q == 0.0 else float(np.sort(sig[finite])[int(tol_q * (finite.sum() - 1))])
        a, _, _ = ac.asks(acc, hist, m2, gx, gy, 16, tolerance=t)
        cnt = ac.tiles_of(a, gx, gy).sum(axis=1)
        for k in (1, 2, 64):
            flags, counts = check_select(hk, acc, hist, m2, st, 16, tolerance=t, tile_pixels=k)
            assert np.array_equal(flags != 0, cnt >= k)
            per_tile.setdefault(k, set()).update(int(c) for c in cnt)
    assert {0, 1, 2} <= per_tile[2] and max(per_tile[64]) < 64            # (the planes' M2 = 0 rows keep every tile below 64 ...)
    # ... so a tile of 64 askers and one of 63 are made: their history zeroed (n = 3 < min_samples), but for one pixel of a row with M2 = 0
    h2 = hist.copy()
    h2[8:24, 8:16] = 0
    h2[17, 12] = 100
    a, few, _ = ac.asks(acc, h2, m2, gx, gy, 3, tolerance=0.0)
    cnt = ac.tiles_of(a, gx, gy).sum(axis=1)
    assert cnt[1 * gy + 1] == 64 and cnt[2 * gy + 1] == 63 and not a[17, 12] and m2[17, 12] == 0
    flags, _ = check_select(hk, acc, h2, m2, st, 3, tolerance=0.0, tile_pixels=64)
    assert flags[1 * gy + 1] == 1 and flags[2 * gy + 1] == 0 and flags.sum() == (cnt == 64).sum()


def test_selection_without_tiles(hk):
    """a grid without a whole tile (38 x 11 and 13 x 9 at divisor 2) selects nothing"""
    for W, H in (pc.TAIL2, pc.TILE):
        acc, hist, m2 = planes(W, H, "wide", True)
        flags, counts = hk.adaptive_select(acc, hist, m2, st_div(2), 4)
        assert len(flags) == 0 and counts["tiles"] == 0 and counts["active_tiles"] == 0 and counts["asking_pixels"] == 0


def test_judge_refuses(hk):
    acc, hist, m2 = planes(*pc.TILE, "mixed", True)
    for divide_by, params in ((-1, {}), (4, {"tolerance": -1.0}), (4, {"tolerance": float("nan")}), (4, {"min_samples": 1}), (4, {"max_samples": 4}),
                              (4, {"max_samples": 3}), (4, {"tile_pixels": 0}), (4, {"tile_pixels": 65})):
        with pytest.raises(RuntimeError, match="adaptive"):
            hk.adaptive_select(acc, hist, m2, ST, divide_by, **params)
    hk.adaptive_select(acc, hist, m2, ST, 0, max_samples=5, tile_pixels=64, tolerance=0.0)


@pytest.mark.parametrize("regions,tiles", [(1, 40), (8, 512), (1, 512), (8, 40), (8, 1)])
def test_split_is_a_stable_partition(hk, regions, tiles):
    rng = np.random.default_rng(1000 * regions + tiles)
    cases_run = 0
    for c in sp.cases(rng, regions, tiles):
        kind, identity, order, rs, emptied = c.kind, c.identity, c.order, c.rs, c.emptied
        flags = sp.flags(c.kept)
        lo, lrs = hk.subset_split(order, c.rs_in(), flags, regions)
        want_lo, want_lrs, _ = sp.partition(order, rs, flags, regions)
        assert np.array_equal(lo, want_lo) and np.array_equal(lrs, want_lrs), (kind, identity, lrs, want_lrs)
        # the properties, plainly: every flagged tile once, the regions' tiles in the order they had, the length in [regions], no split counts
        assert np.array_equal(np.sort(lo), np.nonzero(flags)[0]) and lrs[regions] == flags.sum() and not lrs[regions + 1:].any()
        full = np.arange(tiles, dtype=np.int32) if order is None else order
        for r in range(regions):
            mine = full[rs[r]:rs[r + 1]]
            assert np.array_equal(lo[lrs[r]:lrs[r + 1]], mine[flags[mine] != 0]), (kind, identity, r)
        if kind == "region":
            assert lrs[emptied] == lrs[emptied + 1]
        cases_run += 1
    assert cases_run == 12


def test_fold_equals_the_restatement(hk):
    """sums that wrap, frames above the luma cap, M2 that saturates, a history plane beyond 65535 -- under random masks, all tiles and none"""
    for (W, H), div in VIEWS:
        st = st_div(div)
        gx, gy = ac.grid(st, W, H)
        rng = np.random.default_rng([W, H, div])
        frames = rng.integers(-2 ** 31, 2 ** 31, size=(3, W, H, 3), dtype=np.int64).astype(np.int32)
        frames[1] = rng.integers(-70000, 70000, size=(W, H, 3)).astype(np.int32)
        for name, kind in (("wide", "random"), ("mixed", "random"), ("mixed", "all"), ("wide", "none")):
            acc, hist, m2 = planes(W, H, name, True)
            flags = {"random": (rng.random(gx * gy) < 0.5), "all": np.ones(gx * gy, bool), "none": np.zeros(gx * gy, bool)}[kind].astype(np.uint8)
            want = ac.fold(acc, hist, m2, frames, flags, gx, gy)
            got = hk.adaptive_add(acc.copy(), hist.copy(), m2.copy(), st, frames, np.nonzero(flags)[0].astype(np.int32)[::-1])      # (any order of the list)
            for k, what in enumerate(("sums", "history", "M2")):
                assert np.array_equal(got[k], want[k]), (W, H, div, name, kind, what)
            m = ac.pixel_mask(flags, gx, gy, W, H)
            assert np.array_equal(got[0][~m], acc[~m]) and np.array_equal(got[1][~m], hist[~m]) and np.array_equal(got[2][~m], m2[~m])
            assert np.array_equal(got[1][m], hist[m] + 3)
            if kind != "none" and (W, H) == pc.BIG:                    # the edges are there
                assert (got[2][m] == np.uint64(pc.U64_MAX)).any() and (mc.capped(frames[0])[m]).any()
                wrapped = (acc.astype(np.int64) + frames.astype(np.int64).sum(axis=0))[m]
                assert (np.abs(wrapped) > 2 ** 31).any()


def test_site_rule(hk):
    """launch_state.hpp site_use: a launch over a subset is held, is never split for the sky and takes the subset's pair; without a subset the
    site's own hold_order stands and nothing else changes"""
    assert hk.site_use(False, False) == (False, True, False)
    assert hk.site_use(True, False) == (True, True, False)
    assert hk.site_use(False, True) == (True, False, True)
    assert hk.site_use(True, True) == (True, False, True)
    # what "held" means for the order is order_begin's: a stored order of the same geometry is used, nothing is recorded, nothing grows
    s = hk.LaunchState()
    view = (ST, dict(W=136, H=96, stripe_mod=1, stripe_rem=0, ncols=17, gy=12, regions=1, scene_gen=1, cert_factor=40, cert_levels=1, camera_entry=1, camera_cert=1))
    assert s.order_begin(view, 204, True, True, hk.site_use(False, True)[0]) == (False, False, False)
    before = s.read()
    assert s.order_end((False, False, False), 8) is False
    assert s.read()["order"]["valid"] == before["order"]["valid"] == 0


def test_surface():
    import dogeray_amd as dr
    hdr = open(os.path.join(ROOT, "include", "dogeray_amd.h")).read()
    for sym in ("dr_render_adaptive", "dr_adaptive_defaults", "dr_stats_adaptive_tiles"):
        assert sym in dr.API_SYMBOLS and sym + "(" in hdr
    assert "#define DR_ABI_VERSION 2" in hdr
    assert ctypes.sizeof(dr.DrAdaptiveParams) == 16 and ctypes.sizeof(dr.DrAdaptiveResult) == 40
    for name in ("render_adaptive", "adaptive_tiles", "render_until_adaptive"):
        assert hasattr(dr.Context, name)
    assert hasattr(dr.ProgressiveRenderer, "run_until_adaptive")
    p = dr.DrAdaptiveParams()
    assert dr.lib().dr_adaptive_defaults(ctypes.byref(p)) == 0
    assert (p.tolerance, p.min_samples, p.max_samples, p.tile_pixels) == (1.0, 4, 0, 1) == tuple(ac.DEFAULTS[k] for k in ("tolerance", "min_samples", "max_samples", "tile_pixels"))
    assert not any(s.startswith("dr_group") and "adaptive" in s for s in dr.API_SYMBOLS)
