"""Sky tiles rendered by the lean build's retiring waves (option sky_tiles = 2): the split of value 1, but no sky_tiles_kernel -- the
waves of the persistent kernel take units (sky tile, chunk of frames) from a cursor once all their lanes have retired.  The body is the sky kernel's
and which wave runs it enters no arithmetic, so accumulators, recorded costs and the split must be the same bytes with values 0, 1 and 2.  As in
tests/test_gpu_sky_tiles.py every context forces the lean build (coop_tiles_per_wave = 0) and a view's first launch has two frames or more (a
single-frame launch of a view not seen before computes no table)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import camera_entry_cases as cases
from camera_entry_cases import SEED, SIZES, STRIDE

pytestmark = pytest.mark.gpu

W, H = SIZES[0]
NAMES = ("hf_1", "hf_0.1", "bunny_small", "cube")
VALUES = (0, 1, 2)


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1
    return dogeray_amd


@pytest.fixture(scope="module")
def scenes(dr, synth, tmp_path_factory):
    paths = cases.paths(synth, tmp_path_factory.mktemp("skyinlinegpu"))
    out = {}
    for name in NAMES:
        path, tex = paths[name]
        sc = dr.Scene.load(path, tex); sc.build_bvh()
        s = sc.settings()
        out[name] = {"path": path, "tex": tex, "scene": sc, "settings": s, "st": dr.pack_settings13(s, 1, spp=1)}
    return out


@pytest.fixture(scope="module")
def ctx(dr, scenes):          # scenes first: the generated scenes exist before this process touches the GPU
    c = dr.Context(0)
    c.set_option("coop_tiles_per_wave", 0)
    yield c
    c.close()


def _render(ctx, st, bg, frames=2, seed=SEED, size=(W, H), launches=1, counters=False):
    ctx.enable_counters(counters)
    ctx.stats_reset()
    ctx.accum_reset(*size)
    for k in range(launches):
        ctx.render_accumulate(st, size[0], size[1], bg, seed + 977 * k, STRIDE, frames)
    out = ctx.accum_read().copy()
    stats = ctx.stats()
    ctx.enable_counters(False)
    return out, stats


def _expected_split(ctx):
    codes = ctx.camera_entry()
    return (int((codes == -1).sum()), int((codes != -1).sum())) if len(codes) else (0, 0)


def _same_for_every_value(ctx, st, bg, what, **kw):
    """the accumulators with sky_tiles 0, 1 and 2 are the same bytes and 1 and 2 report the table's split; returns that split"""
    got, split = {}, {}
    for v in VALUES:
        ctx.set_option("sky_tiles", v)
        got[v], _ = _render(ctx, st, bg, **kw)
        split[v] = ctx.sky_tiles()
        assert split[v] == (_expected_split(ctx) if v else (0, 0)), (what, v)
    assert np.array_equal(got[1], got[0]), what
    assert np.array_equal(got[2], got[0]), what
    assert split[2] == split[1], what
    return split[2]


def _spp(st, spp):
    out = np.array(st, np.float32).copy()
    out[10] = spp
    return out


def _turned(st, degrees):
    """the view turned about the vertical axis through the eye"""
    out = np.array(st, np.float32).copy()
    a = np.deg2rad(degrees)
    d = out[3:6] - out[0:3]
    out[3] = out[0] + np.float32(np.cos(a) * d[0] + np.sin(a) * d[2])
    out[5] = out[2] + np.float32(-np.sin(a) * d[0] + np.cos(a) * d[2])
    return out


@pytest.mark.parametrize("frames", [2, 3, 9])
@pytest.mark.parametrize("name", ["hf_1", "bunny_small", "cube"])
def test_accumulators_are_the_same_for_every_value(ctx, scenes, name, frames):
    """hf_small from its own view and from above, bunny_small (no sky tile), the cube; both sizes; one and two samples"""
    e = scenes[name]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    sky = 0
    for size in SIZES:
        for v in cases.views(name, e["st"]):
            for spp in (1, 2):
                sky += _same_for_every_value(ctx, _spp(v, spp), bg, (name, frames, size, spp), frames=frames, size=size)[0]
    assert (sky > 0) == (name != "bunny_small"), name


def test_eight_regions_and_the_feedback_order(ctx, scenes):
    """256 x 128: 512 tiles, a queue per XCD.  Three launches of one view; the second and the third (one frame each: only a one-frame launch's costs are
    the same from run to run) run on an order made from a split launch's costs.  The costs the order after the third launch was made from -- the
    second launch's -- are the same words with values 1 and 2 (and 0), the order is the plain reference's order of those costs with either, and so
    are the accumulators."""
    import tile_order_checks as tc
    e = scenes["hf_0.1"]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    size = (256, 128)
    got = {}
    for v in VALUES:
        ctx.set_option("heavy_factor", 1)                                  # (setting it drops the stored order: every run starts from the identity)
        ctx.set_option("sky_tiles", v)
        ctx.accum_reset(*size)
        ctx.render_accumulate(e["st"], size[0], size[1], bg, SEED, STRIDE, 2)
        ctx.render_accumulate(e["st"], size[0], size[1], bg, SEED + 977, STRIDE, 1)
        cost = ctx.pixel_cost(size[0], size[1], raw=True).copy()
        ctx.render_accumulate(e["st"], size[0], size[1], bg, SEED + 977 * 2, STRIDE, 1)
        acc = ctx.accum_read().copy()
        split = ctx.sky_tiles()
        order = ctx.tile_order()
        assert order is not None and order["regions"] == 8 and order["ntiles"] == 512
        assert split == (_expected_split(ctx) if v else (0, 0))
        ref = tc.Reference(tc.tile_cost(cost, 512), 8, 1, order["split_steps"], order["split_limit"])
        assert tc.first_difference(ref, order["order"], order["region_start"]) is None, v
        got[v] = (acc, cost, split)
    assert got[2][2][0] > 0 and got[2][2][1] > 0 and got[2][2] == got[1][2]
    for v in (1, 2):
        assert np.array_equal(got[v][0], got[0][0]), v
        assert len(got[v][1]) == 512 * 64 and np.array_equal(got[v][1], got[0][1]), v
    codes = ctx.camera_entry()
    assert not got[2][1].reshape(512, 64)[codes == -1].any()               # a sky tile's pixels cost 0 node steps


def test_a_stripe(ctx, scenes):
    e = scenes["hf_0.1"]
    ctx.upload(e["scene"])
    ctx.set_stripe(2, 1)
    try:
        sky = 0
        for st in cases.views("hf_0.1", e["st"]):
            split = _same_for_every_value(ctx, st, e["settings"].background, "stripe", size=SIZES[1], frames=3)
            assert split[0] + split[1] == 4 * 5                            # block columns 1, 3, 5, 7 of nine
            sky += split[0]
        assert sky > 0
    finally:
        ctx.set_stripe(1, 0)


def test_a_view_of_nothing_but_sky(ctx, scenes):
    """every tile is a sky tile: the queues are empty at a wave's first look and it goes straight to the units"""
    e = scenes["cube"]
    ctx.upload(e["scene"])
    st = _turned(cases.lens(e["st"], 0), 75.0)
    for frames in (2, 9):
        assert _same_for_every_value(ctx, st, e["settings"].background, "turned away", frames=frames) == ((W // 8) * (H // 8), 0)


def test_a_moved_view_straight_after(ctx, scenes):
    e = scenes["hf_0.1"]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    for k in range(3):
        st = cases.top("hf_0.1", e["st"])
        st[0] += np.float32(0.07 * k); st[2] += np.float32(0.05 * k)       # every launch a new view, right after the last
        assert _same_for_every_value(ctx, st, bg, k, seed=11 + k)[0] > 0


def test_a_second_launch_of_one_frame(ctx, scenes):
    """two frames (the view's table, atomic adds), then one frame of the same view in a launch of its own: the plain += of P.accumulate = 1"""
    e = scenes["hf_0.1"]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    st = cases.top("hf_0.1", e["st"])
    got = {}
    for v in VALUES:
        ctx.set_option("sky_tiles", v)
        ctx.accum_reset(W, H)
        ctx.render_accumulate(st, W, H, bg, SEED, STRIDE, 2)
        two = ctx.accum_read().copy()
        ctx.render_accumulate(st, W, H, bg, SEED + 977, STRIDE, 1)
        assert ctx.sky_tiles() == (_expected_split(ctx) if v else (0, 0)) and (ctx.sky_tiles()[0] > 0) == (v > 0)
        got[v] = (two, ctx.accum_read().copy())
    for v in (1, 2):
        assert np.array_equal(got[v][0], got[0][0]) and np.array_equal(got[v][1], got[0][1]), v
    assert not np.array_equal(got[0][0], got[0][1])


def test_one_frame_stored(ctx, scenes):
    """dr_render_frame (a store, not an add) of a view whose table exists, through the lean build"""
    e = scenes["cube"]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    st = cases.lens(e["st"], 0)
    ctx.set_option("coop_steps", 0)
    try:
        got = {}
        for v in VALUES:
            ctx.set_option("sky_tiles", v)
            _render(ctx, st, bg, 2)                                        # the view's table (the option dropped it)
            got[v] = ctx.render_frame(st, W, H, bg, SEED + 3).copy()
            codes = ctx.camera_entry()
            assert len(codes) and (codes == -1).any()
            assert ctx.sky_tiles() == (_expected_split(ctx) if v else (0, 0))
        assert np.array_equal(got[1], got[0]) and np.array_equal(got[2], got[0])
    finally:
        ctx.set_option("coop_steps", 2)


def test_many_launches_cross_the_wrap_of_the_counters(ctx, scenes):
    """forty calls of three launches each on one context: every launch takes a block of the tile counters (a cursor per queue and the units' cursor),
    and the blocks wrap -- cleared on the stream -- after some 110 launches.  A cursor that did not start at zero would leave sky tiles unrendered."""
    e = scenes["hf_0.1"]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    st = cases.top("hf_0.1", e["st"])
    ctx.set_option("batch_frames", 2)
    try:
        got = {}
        for v in (1, 2):
            ctx.set_option("sky_tiles", v)
            ctx.accum_reset(W, H)
            for k in range(40):
                ctx.render_accumulate(st, W, H, bg, SEED + 977 * k, STRIDE, 6)
            assert ctx.sky_tiles()[0] > 0
            got[v] = ctx.accum_read().copy()
        assert np.array_equal(got[2], got[1])
    finally:
        ctx.set_option("batch_frames", 32)


def test_the_counting_build_is_not_split(ctx, scenes):
    e = scenes["hf_0.1"]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    st = cases.top("hf_0.1", e["st"])
    ctx.set_option("sky_tiles", 2)
    on, so = _render(ctx, st, bg, 2, counters=True)
    assert ctx.sky_tiles() == (0, 0) and (ctx.camera_entry() == -1).any()
    ctx.set_option("sky_tiles", 0)
    off, sf = _render(ctx, st, bg, 2, counters=True)
    assert np.array_equal(on, off)
    assert so["rays"] == sf["rays"] > 0 and so["samples"] == sf["samples"] > 0
    ctx.set_option("sky_tiles", 2)
    lean, _ = _render(ctx, st, bg, 2)
    assert ctx.sky_tiles()[0] > 0 and np.array_equal(lean, on)


def test_frames_equal_the_oracle(ctx, scenes):
    from oracle import orc
    e = scenes["hf_0.1"]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    st = cases.views("hf_0.1", e["st"])[-1]
    ctx.set_option("sky_tiles", 2)
    got, _ = _render(ctx, st, bg, 2)
    assert ctx.sky_tiles()[0] > 0
    o = orc.Scene(e["path"], e["tex"] or None); o.build_bvh()
    want = sum(o.render(st, W, H, bg, SEED + STRIDE * k, nthreads=8)[0].astype(np.int64) for k in range(2))
    assert np.array_equal(got.astype(np.int64), want)
