"""Option sample_order on the GPU (launch_plan.hpp tile_sample): with 1 a unit of the persistent kernel's queue is consecutive frames of
one or two pixels of its tile instead of the tile's 64 pixels of one frame.  A pixel's arithmetic depends on (x, y, frame) only and a batch is summed
with integer adds, so a launch of B frames must give the same bytes with either order, and the bytes of B launches of one frame.

The suite's small height field at 64 x 48 (48 tiles) and golden/scenes/mats.rts; the frames of a scene rendered one per launch are summed once, as
prefix sums, and shared.  Unless a test says otherwise the context forces the lean build (coop_tiles_per_wave = 0), as tests/test_gpu_sky_inline.py
does.  Every comparison is integer equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import SCENES

pytestmark = pytest.mark.gpu

W, H = 64, 48
TILES = (W // 8) * (H // 8)
SEED, STRIDE = 23, 1000003
BATCHES = (1, 2, 3, 20, 32, 63, 64, 65, 256)
RESTORE = (("sample_order", 1), ("batch_frames", 32), ("coop_tiles_per_wave", 0), ("wave_log", 0), ("pipe_group", 8))


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


@pytest.fixture(scope="module")
def world(dr, synth):          # synth first: the generated scenes exist before this process touches the GPU
    w = {"scene": {}, "st": {}, "bg": {}}
    for name, path in (("hf", os.path.join(synth["dir"], "hf_small.rts")), ("mats", os.path.join(SCENES, "mats.rts"))):
        sc = dr.Scene.load(path, ""); sc.build_bvh()
        s = sc.settings()
        w["scene"][name], w["st"][name], w["bg"][name] = sc, dr.pack_settings13(s, 1, spp=1), s.background
    c = dr.Context(0)
    assert c.get_option("sample_order") in (0, 1)
    w["ctx"], w["loaded"], w["singles"] = c, None, {}
    yield w
    c.close()


@pytest.fixture()
def ctx(world):
    c = world["ctx"]
    for name, value in RESTORE:
        c.set_option(name, value)
    try:
        yield c
    finally:
        for name, value in RESTORE:
            c.set_option(name, value)
        c.set_stripe(1, 0)
        c.enable_counters(False)


def _load(world, name):
    if world["loaded"] != name:
        world["ctx"].upload(world["scene"][name])
        world["loaded"] = name


def _spp(st, spp):
    out = np.array(st, np.float32).copy()
    out[10] = spp
    return out


def _batch(c, st, bg, B, order, seed=SEED):
    """one launch of B frames with this sample order: the accumulator"""
    c.set_option("sample_order", order)
    c.set_option("batch_frames", B)
    c.stats_reset()
    c.accum_reset(W, H)
    c.render_accumulate(st, W, H, bg, seed, STRIDE, B)
    assert c.stats()["launches"] == 1
    return c.accum_read().copy()


def _singles(world, name, st, stripe=(1, 0), upto=max(BATCHES), at=BATCHES):
    """B -> the sum of frames 0 .. B - 1 of this scene and view, one frame per launch (batch_frames 1: both orders are the identity); rendered once"""
    key = (name, np.asarray(st, np.float32).tobytes(), stripe)
    if key not in world["singles"]:
        c = world["ctx"]
        c.set_option("batch_frames", 1)
        c.stats_reset()
        c.accum_reset(W, H)
        sums = {}
        for k in range(upto):
            c.render_accumulate(st, W, H, world["bg"][name], SEED + STRIDE * k, STRIDE, 1)
            if k + 1 in at:
                a = c.accum_read().copy()
                a.flags.writeable = False
                sums[k + 1] = a
        assert c.stats()["launches"] == upto
        world["singles"][key] = sums
    return world["singles"][key]


def _differ(a, b):
    return "%d pixels differ" % int((a != b).any(axis=2).sum())


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", ["hf", "mats"])
def test_both_orders_and_single_launches_are_the_same_bytes(world, ctx, name, B):
    _load(world, name)
    st, bg = world["st"][name], world["bg"][name]
    want = _singles(world, name, st)[B]
    assert want.any()
    zero, one = _batch(ctx, st, bg, B, 0), _batch(ctx, st, bg, B, 1)
    assert np.array_equal(one, zero), "order 1 against order 0: " + _differ(one, zero)
    assert np.array_equal(one, want), "order 1 against %d launches of one frame: %s" % (B, _differ(one, want))


def test_a_stripe(world, ctx):
    """block columns 1, 4, 7 of eight: the tile's column is the stripe's, the pixel still the sample order's"""
    _load(world, "hf")
    st, bg = world["st"]["hf"], world["bg"]["hf"]
    ctx.set_stripe(3, 1)
    want = _singles(world, "hf", st, stripe=(3, 1), upto=20, at=(20,))[20]
    whole = _singles(world, "hf", st)[20]
    assert want.any() and not np.array_equal(want, whole), "the stripe hides nothing"
    ctx.set_stripe(3, 1)
    zero, one = _batch(ctx, st, bg, 20, 0), _batch(ctx, st, bg, 20, 1)
    assert np.array_equal(one, zero), _differ(one, zero)
    assert np.array_equal(one, want), _differ(one, want)


def test_a_pipelined_group_stores_every_sample_in_its_own_frame(world, ctx):
    """eight frames submitted to the pipeline are one launch that stores each frame into a buffer of its own; the image of ticket k is that of the sum of
    frames 0 .. k, so a sample stored into another frame's buffer, twice or not at all shows in one of them"""
    _load(world, "hf")
    st, bg = world["st"]["hf"], world["bg"]["hf"]
    ref = world["ctx"]
    frames = [ref.render_frame(st, W, H, bg, SEED + STRIDE * k).astype(np.int64) for k in range(8)]
    assert not np.array_equal(frames[0], frames[1])
    ctx.set_option("coop_tiles_per_wave", 32)
    for order in (0, 1):
        ctx.set_option("sample_order", order)
        ctx.stats_reset()
        ctx.accum_reset(W, H)
        tickets = [ctx.pipeline_submit(st, W, H, bg, SEED + STRIDE * k, present_divide_by=k + 1) for k in range(8)]
        total = np.zeros((W, H, 3), dtype=np.int64)
        for k, t in enumerate(tickets):
            total = total + frames[k]
            got = ctx.pipeline_wait(t, want_image=True)
            want = np.clip((np.abs(total) // (k + 1)) * np.sign(total), 0, 255).astype(np.uint8).transpose(1, 0, 2)
            assert np.array_equal(got, want), "order %d, image of frame %d: %d pixels differ" % (order, k, int((got != want).any(axis=2).sum()))
        assert np.array_equal(ctx.accum_read().astype(np.int64), total), order
        s = ctx.stats()
        assert (s["frames"], s["launches"]) == (8, 1), "the eight frames were not one group"


def test_the_counting_build(world, ctx):
    _load(world, "hf")
    st, bg = world["st"]["hf"], world["bg"]["hf"]
    got = {}
    for order in (0, 1):
        ctx.enable_counters(True)
        acc = _batch(ctx, st, bg, 20, order)
        s = ctx.stats()
        ctx.enable_counters(False)
        assert s["samples"] == W * H * 20, (order, s["samples"])
        got[order] = (acc, s)
    for key in ("rays", "node_visits", "prim_tests"):
        assert got[1][1][key] == got[0][1][key] > 0, key
    assert np.array_equal(got[1][0], got[0][0]) and np.array_equal(got[1][0], _singles(world, "hf", st)[20])


def test_the_work_sharing_build(world, ctx):
    """48 tiles x 3 frames are few units per wave: the plan picks the work-sharing build, the only one that writes the wave log"""
    _load(world, "hf")
    st, bg = world["st"]["hf"], world["bg"]["hf"]
    ctx.set_option("coop_tiles_per_wave", 32)
    ctx.set_option("wave_log", 1)
    zero = _batch(ctx, st, bg, 3, 0)
    assert len(ctx.wave_log()) > 0, "not the work-sharing build"
    one = _batch(ctx, st, bg, 3, 1)
    assert len(ctx.wave_log()) > 0, "not the work-sharing build"
    assert np.array_equal(one, zero), _differ(one, zero)
    assert np.array_equal(one, _singles(world, "hf", st)[3])


def test_two_samples_per_pixel(world, ctx):
    """the second sample of a pixel is rendered by the lane that rendered the first, for the same frame"""
    _load(world, "hf")
    st, bg = _spp(world["st"]["hf"], 2), world["bg"]["hf"]
    want = _singles(world, "hf", st, upto=3, at=(3,))[3]
    assert not np.array_equal(want, _singles(world, "hf", world["st"]["hf"])[3])
    zero, one = _batch(ctx, st, bg, 3, 0), _batch(ctx, st, bg, 3, 1)
    assert np.array_equal(one, zero), _differ(one, zero)
    assert np.array_equal(one, want), _differ(one, want)


@pytest.mark.parametrize("what, index", [("depth limit 0", 9), ("no samples", 10)])
def test_a_degenerate_launch(world, ctx, what, index):
    """A launch that traces nothing (depth limit 0, or a sample count of 0) still takes every pixel of every frame and stores it, black: every lane
    with a pixel stores in its first phase -- the densest merge the kernel can produce, a whole wave of the frames of one or two pixels at once.  The
    stores add zeros, so they are made on top of one ordinary frame: the accumulator of a batch of 20 is that of 20 launches of one frame, which is
    that frame's, with either order, in the lean and in the counting build -- and the counting build's samples say that the pixels were taken."""
    _load(world, "hf")
    st, bg = world["st"]["hf"], world["bg"]["hf"]
    nothing = np.array(st, np.float32).copy()
    nothing[index] = 0

    def run(B, launches, order, counting):
        ctx.set_option("sample_order", order)
        ctx.set_option("batch_frames", 1)
        ctx.accum_reset(W, H)
        ctx.render_accumulate(st, W, H, bg, SEED, STRIDE, 1)
        ctx.set_option("batch_frames", B)
        ctx.enable_counters(counting)
        ctx.stats_reset()
        for k in range(launches):
            ctx.render_accumulate(nothing, W, H, bg, SEED + STRIDE * (1 + k * B), STRIDE, B)
        s = ctx.stats()
        ctx.enable_counters(False)
        assert s["launches"] == launches, (what, B, order, s["launches"])
        if counting:
            assert s["samples"] == W * H * 20 and s["rays"] == 0, (what, B, order, s["samples"], s["rays"])
        return ctx.accum_read().copy()

    frame = _singles(world, "hf", st)[1]
    assert frame.any()
    for counting in (False, True):
        want = run(1, 20, 1, counting)
        assert np.array_equal(want, frame), "%s: 20 launches of one frame changed the accumulator: %s" % (what, _differ(want, frame))
        for order in (0, 1):
            got = run(20, 1, order, counting)
            assert np.array_equal(got, want), "%s, order %d, counting %s: %s" % (what, order, counting, _differ(got, want))


def test_pixel_cost_is_indexed_by_the_pixel(world, ctx):
    """A pixel's recorded cost is the node steps of one of its frames (the frames of a launch write the same word: the last one stays).  After a launch
    of three frames with order 1 every word is the cost the same pixel has in a single launch of one of the three, and it is zero exactly on the
    pixels that walked nothing: those of the tiles whose entry code says no leaf can be seen."""
    _load(world, "hf")
    st, bg = world["st"]["hf"], world["bg"]["hf"]
    _batch(ctx, st, bg, 2, 1)                                   # the view's entry table: the launches below all start their camera rays from it
    each = []
    for k in range(3):
        _batch(ctx, st, bg, 1, 1, seed=SEED + STRIDE * k)
        each.append(ctx.pixel_cost(W, H, raw=True).copy())
    _batch(ctx, st, bg, 3, 1)
    cost = ctx.pixel_cost(W, H, raw=True).copy()
    codes = ctx.camera_entry()
    assert len(cost) == TILES * 64 and len(codes) == TILES and (codes != -1).any()
    assert np.mean(each[0] != each[1]) > 0.25, "the frames' costs are too alike to tell a pixel from its neighbour"
    walked = np.repeat(codes != -1, 64)
    assert np.array_equal(cost != 0, walked), "%d words" % int(((cost != 0) != walked).sum())
    member = (cost == each[0]) | (cost == each[1]) | (cost == each[2])
    assert member.all(), "%d of %d words are not the pixel's cost in any of its three frames" % (int((~member).sum()), len(cost))
