"""The kernel that splits a launch's tile order (kernels_aux.hip order_split_kernel, both instances) on the GPU against the plain function that defines
its arrays (device_split.hpp order_split_plain, through the host build's hk_sky_split / hk_subset_split): every case of tests/split_cases.py through
dr_kat_order_split, every array compared exactly -- the kept tiles in their order, all 17 words of the region starts, the dropped list, the counts --
and what lies behind the lists still the 0xff preset.  The tile counts are where this kernel can go wrong: one group and its edges (1, 40, 63, 64,
65), whole and ragged ranges of the 16 waves with empty ones behind (512, 1 023, 1 025), the first count whose ranges exceed one round trip of
8 x 64 loads (8 193), and the 1920 x 1080 view's 32 400.  Each case is one launch of one workgroup.  The hook's refusals are host checks: nothing is
launched for them."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import split_cases as sp

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

I, U32 = np.int32, np.uint32
TILES = (1, 40, 63, 64, 65, 512, 1023, 1025, 8193, 32400)
SKY, FLAG = 0, 1


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.fixture(scope="module")
def ctx(dr, hk):          # hk first: the host build exists before this process touches the GPU
    c = dr.Context(0)
    yield c
    c.close()


def check(ctx, hk, kind, c, key, regions, where):
    tiles = len(c.kept)
    lo, lrs, dl, counts = ctx.kat_order_split(kind, regions, c.order, c.rs_in(), key)
    if kind == SKY:
        want_lo, want_lrs, want_dl = hk.sky_split(c.order, c.rs_in(), key, regions)
    else:
        (want_lo, want_lrs), want_dl = hk.subset_split(c.order, c.rs_in(), key, regions), np.zeros(0, I)
    kept, dropped = len(want_lo), len(want_dl)
    assert kept == int(c.kept.sum()) and lo.shape == (tiles,) and dl.shape == (tiles,), where
    assert np.array_equal(lo[:kept], want_lo), (where, "launch_order")
    assert np.array_equal(lrs, want_lrs), (where, lrs, want_lrs)
    assert np.array_equal(dl[:dropped], want_dl), (where, "dropped_list")
    assert (lo[kept:] == -1).all() and (dl[dropped:] == -1).all(), (where, "the preset behind the lists")
    if kind == SKY:
        assert dropped == tiles - kept and counts.tolist() == [dropped, kept], (where, counts)
    else:
        assert counts.tolist() == [0xffffffff] * 2, (where, counts)      # no list, no counts: the preset


@pytest.mark.parametrize("regions", (1, 8))
@pytest.mark.parametrize("tiles", TILES)
def test_the_kernel_writes_what_the_plain_function_writes(ctx, hk, tiles, regions):
    """both instances over the twelve cases: permuted orders with random cuts (empty regions, regions that start at ntiles) and the identity with
    make_params' bands"""
    rng = np.random.default_rng(10 * tiles + regions)
    n = 0
    for c in sp.cases(rng, regions, tiles):
        where = (tiles, regions, c.kind, c.identity)
        check(ctx, hk, SKY, c, sp.words(rng, c.kept), regions, where + ("words",))
        check(ctx, hk, FLAG, c, sp.flags(c.kept), regions, where + ("flags",))
        n += 1
    assert n == 12


def test_regions_that_start_at_the_end(ctx, hk):
    """eight regions of which the last five are empty and start at ntiles, the first tiles all dropped: starts the kernel fixes up after the placing"""
    tiles = 1025
    rs = np.array([0, 0, 700, 1025, 1025, 1025, 1025, 1025, 1025], I)
    rng = np.random.default_rng(5)
    for order in (None, rng.permutation(tiles).astype(I)):
        kept = rng.random(tiles) < 0.5
        kept[(np.arange(tiles, dtype=I) if order is None else order)[:64]] = False
        c = sp.Case("cuts", order is None, order, rs, kept, None)
        check(ctx, hk, SKY, c, sp.words(rng, kept), 8, ("ends", order is None, "words"))
        check(ctx, hk, FLAG, c, sp.flags(kept), 8, ("ends", order is None, "flags"))


def test_refusals(dr, ctx):
    """what the kernel relies on is judged on the host, before any launch"""
    n = 100
    order, rs, word, flag = np.arange(n, dtype=I)[::-1].copy(), np.array([0, 30, 30, 100], I), np.zeros(n, U32), np.ones(n, np.uint8)
    twice, beyond, negative = order.copy(), order.copy(), order.copy()
    twice[3] = twice[4]; beyond[0] = n; negative[n - 1] = -1
    bad = [(2, 3, order, rs, word), (-1, 3, order, rs, word),                                        # kind
           (0, 0, order, rs, word), (0, 9, order, np.arange(10, dtype=I) * 0 + 100, word), (1, -1, order, rs, flag),      # regions
           (0, 3, order, np.array([1, 30, 30, 100], I), word), (1, 3, order, np.array([0, 30, 30, 99], I), flag),      # the ends of region_start
           (0, 3, order, np.array([0, 31, 30, 100], I), word), (1, 3, None, np.array([0, 30, 101, 100], I), flag),      # ... not non-decreasing
           (0, 3, twice, rs, word), (1, 3, beyond, rs, flag), (0, 3, negative, rs, word)]           # no permutation
    for kind, regions, o, r, key in bad:
        with pytest.raises(dr.DogerayError) as e:
            ctx.kat_order_split(kind, regions, o, r, key)
        assert e.value.code == dr.ERR_INVALID, (kind, regions)
    for kind, key in ((0, np.zeros(0, U32)), (1, np.zeros(0, np.uint8))):                           # no empty call
        with pytest.raises(dr.DogerayError) as e:
            ctx.kat_order_split(kind, 1, None, np.array([0, 0], I), key)
        assert e.value.code == dr.ERR_INVALID
    lo, lrs, dl, counts = ctx.kat_order_split(0, 3, order, rs, word)                                # and the well-formed call next to them is served
    assert np.array_equal(lo, order) and lrs[:4].tolist() == [0, 30, 30, 100] and counts.tolist() == [0, n]
