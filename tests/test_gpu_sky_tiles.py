"""Sky tiles on the GPU (option sky_tiles): a lean launch over a view with an entry table renders the tiles of entry code -1 in
sky_tiles_kernel and hands the persistent kernel the rest of its order.  Only the lean build is split and a single-frame launch of a view not seen
before computes no table, so every context here forces the lean build (coop_tiles_per_wave = 0) and launches two frames or more.  Accumulators must
be byte-identical with sky_tiles 1 and 0; the split must count the table's -1 codes; the counting build must not be split."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import camera_entry_cases as cases
from camera_entry_cases import SEED, STRIDE

pytestmark = pytest.mark.gpu

W, H = 64, 40
NAMES = ("hf_0.1", "hf_1", "cube", "tiny_2", "matball", "bunny_small")


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1
    return dogeray_amd


@pytest.fixture(scope="module")
def scenes(dr, synth, tmp_path_factory):
    """name -> the device's scene, its settings, and settings13 at one sample per pixel"""
    paths = cases.paths(synth, tmp_path_factory.mktemp("skygpu"))
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
    c.set_option("coop_tiles_per_wave", 0)      # every launch runs the lean build (six waves per SIMD), or the counting build when counters are on
    yield c
    c.close()


def _render(ctx, st, bg, frames=2, seed=SEED, counters=False, size=(W, H), launches=1, **options):
    for k, v in options.items(): ctx.set_option(k, v)
    ctx.enable_counters(counters)
    ctx.stats_reset()
    ctx.accum_reset(*size)
    for k in range(launches):
        ctx.render_accumulate(st, size[0], size[1], bg, seed + 977 * k, STRIDE, frames)
    out = ctx.accum_read().copy()
    stats = ctx.stats()
    ctx.enable_counters(False)
    return out, stats


LAST = {}      # "codes": the entry codes of _on_off's launch with the feature on


def _on_off(ctx, st, bg, what, **kw):
    """the accumulators with the feature on and off are the same bytes; returns the one rendered with it on and the split's (sky, geometry) counts"""
    on, _ = _render(ctx, st, bg, sky_tiles=1, **kw)
    split = ctx.sky_tiles()
    codes = ctx.camera_entry()
    LAST["codes"] = codes
    if len(codes):
        assert split == (int((codes == -1).sum()), int((codes != -1).sum())), what
    else:
        assert split == (0, 0), what                      # no table: the launch is not split
    off, _ = _render(ctx, st, bg, sky_tiles=0, **kw)
    assert ctx.sky_tiles() == (0, 0), what
    assert np.array_equal(on, off), what
    ctx.set_option("sky_tiles", 1)
    return on, split


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


@pytest.mark.parametrize("spp", [1, 2])
@pytest.mark.parametrize("frames", [2, 3])
@pytest.mark.parametrize("name", ["hf_0.1", "hf_1", "cube", "tiny_2", "matball"])
def test_accumulators_do_not_depend_on_the_split(ctx, scenes, name, frames, spp):
    e = scenes[name]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    sky = 0
    for v in cases.views(name, e["st"]):
        for k in (0, 1):                                                   # the lens closed, and the scene's own
            _, split = _on_off(ctx, _spp(cases.lens(v, k), spp), bg, (name, frames, spp, k), frames=frames)
            sky += split[0]
    print("%s: %d sky tiles over the views" % (name, sky))
    assert sky > 0, name


def test_eight_regions_and_the_feedback_order(ctx, scenes):
    """512 tiles: one queue per XCD.  Three launches of one view: the second and the third run on an order made from the costs of a split launch.  The
    order after the third launch is the one made from the second launch's costs (the third refreshes nothing): those costs must be the same words with
    the feature on and off, and both orders must be the order of those costs.  (The second and third launch are of one frame: the frames of a batch
    record a pixel's cost into the same word, whichever finishes last, so only a one-frame launch's costs are the same from run to run.)  (Inside a cost class the device places heavy tiles with atomics, in any
    order -- DESIGN.md 4.3, tests/tile_order_checks.py --, so two orders of the same costs are compared as tests/test_gpu_tile_order.py compares them:
    through the plain reference, every class's run sorted by tile number.)"""
    import tile_order_checks as tc
    e = scenes["hf_0.1"]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    size = (256, 128)
    for heavy in (1, -1):
        got = {}
        for sky in (1, 0):
            ctx.set_option("heavy_factor", heavy)                          # (setting it drops the stored order: both runs start from the identity)
            ctx.set_option("sky_tiles", sky)
            ctx.accum_reset(*size)
            ctx.render_accumulate(e["st"], size[0], size[1], bg, SEED, STRIDE, 2)                # the view's table
            ctx.render_accumulate(e["st"], size[0], size[1], bg, SEED + 977, STRIDE, 1)
            cost = ctx.pixel_cost(size[0], size[1], raw=True).copy()      # the second launch's: what the order is made from
            ctx.render_accumulate(e["st"], size[0], size[1], bg, SEED + 977 * 2, STRIDE, 1)
            acc = ctx.accum_read().copy()
            split = ctx.sky_tiles()
            order = ctx.tile_order()
            assert order is not None and order["regions"] == 8 and order["ntiles"] == 512 and order["heavy_factor"] == heavy
            codes = ctx.camera_entry()
            assert split == ((int((codes == -1).sum()), int((codes != -1).sum())) if sky else (0, 0))
            ref = tc.Reference(tc.tile_cost(cost, 512), 8, heavy, order["split_steps"], order["split_limit"])
            assert tc.first_difference(ref, order["order"], order["region_start"]) is None, (heavy, sky)
            got[sky] = (acc, cost, split)
        assert got[1][2][0] > 0 and got[1][2][1] > 0
        assert np.array_equal(got[1][0], got[0][0]), heavy
        assert len(got[1][1]) == 512 * 64 and np.array_equal(got[1][1], got[0][1]), heavy
    ctx.set_option("heavy_factor", 1); ctx.set_option("sky_tiles", 1)


def test_a_stripe(ctx, scenes):
    e = scenes["hf_0.1"]
    ctx.upload(e["scene"])
    ctx.set_stripe(2, 1)
    try:
        sky = 0
        for st in cases.views("hf_0.1", e["st"]):
            _, split = _on_off(ctx, st, e["settings"].background, "stripe", size=(72, 44))
            assert split[0] + split[1] == 4 * 5                            # block columns 1, 3, 5, 7 of nine
            sky += split[0]
        assert sky > 0
    finally:
        ctx.set_stripe(1, 0)


def test_a_scene_without_sky_tiles(ctx, scenes):
    e = scenes["bunny_small"]                                              # its floor reaches behind the lens: every tile at the root
    ctx.upload(e["scene"])
    _, split = _on_off(ctx, e["st"], e["settings"].background, "bunny_small")
    assert split == (0, (W // 8) * (H // 8))


def test_a_view_of_nothing(ctx, scenes):
    """the cube well outside the frustum but in front of the lens plane: every tile is a sky tile and the persistent kernel's queues are empty"""
    e = scenes["cube"]
    ctx.upload(e["scene"])
    st = _turned(cases.lens(e["st"], 0), 75.0)
    on, split = _on_off(ctx, st, e["settings"].background, "turned away", frames=3)
    assert split == ((W // 8) * (H // 8), 0)
    assert bool(on.any()) == (e["settings"].background > 0)                # the sky


def test_a_moved_view_straight_after(ctx, scenes):
    e = scenes["hf_0.1"]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    seen = set()
    for k in range(3):
        st = cases.top("hf_0.1", e["st"])
        st[0] += np.float32(0.07 * k); st[2] += np.float32(0.05 * k)       # the eye moves over the field: every launch a new view, right after the last
        _, split = _on_off(ctx, st, bg, k, seed=11 + k)
        seen.add(LAST["codes"].tobytes())
        assert split[0] > 0
    assert len(seen) == 3


def test_one_frame_stored(ctx, scenes):
    """dr_render_frame (a store, not an add) of a view whose table exists, through the lean build"""
    e = scenes["cube"]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    st = cases.lens(e["st"], 0)
    ctx.set_option("coop_steps", 0)
    try:
        _render(ctx, st, bg, 2, sky_tiles=1)                               # the view's table
        got = {}
        for sky in (1, 0):
            ctx.set_option("sky_tiles", sky)
            _render(ctx, st, bg, 2)                                        # (the option dropped the table)
            got[sky] = ctx.render_frame(st, W, H, bg, SEED + 3).copy()
            split = ctx.sky_tiles()
            codes = ctx.camera_entry()
            assert len(codes) and (codes == -1).any()
            assert split == ((int((codes == -1).sum()), int((codes != -1).sum())) if sky else (0, 0))
        assert np.array_equal(got[1], got[0])
    finally:
        ctx.set_option("coop_steps", 2); ctx.set_option("sky_tiles", 1)


def test_the_counting_build_is_not_split(ctx, scenes):
    e = scenes["hf_0.1"]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    st = cases.top("hf_0.1", e["st"])
    on, so = _render(ctx, st, bg, 2, counters=True, sky_tiles=1)
    assert ctx.sky_tiles() == (0, 0) and (ctx.camera_entry() == -1).any()
    off, sf = _render(ctx, st, bg, 2, counters=True, sky_tiles=0)
    assert np.array_equal(on, off)
    assert so["rays"] == sf["rays"] > 0 and so["samples"] == sf["samples"] > 0
    lean, _ = _render(ctx, st, bg, 2, sky_tiles=1)
    assert ctx.sky_tiles()[0] > 0 and np.array_equal(lean, on)


def test_frames_with_sky_tiles_equal_the_oracle(ctx, scenes):
    from oracle import orc
    for name in ("hf_0.1", "cube"):
        e = scenes[name]
        ctx.upload(e["scene"])
        bg = e["settings"].background
        st = cases.views(name, e["st"])[-1]
        got, _ = _render(ctx, st, bg, 2, sky_tiles=1)
        assert ctx.sky_tiles()[0] > 0, name
        o = orc.Scene(e["path"], e["tex"] or None); o.build_bvh()
        want = sum(o.render(st, W, H, bg, SEED + STRIDE * k, nthreads=8)[0].astype(np.int64) for k in range(2))
        assert np.array_equal(got.astype(np.int64), want), name
