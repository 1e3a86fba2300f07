"""The tile-order feedback kernels (kernels_aux.hip tile_cost_kernel, tile_order_kernel) on the GPU against the plain reference of
tests/tile_order_checks.py: every case of tests/tile_order_cases.py through dr_kat_tile_feedback, the live order of a context through
dr_stats_tile_order, and the pixels of a frame size whose order takes the kernel's multi-group paths (8320 tiles, eight regions) against the
oracle.  tests/test_tile_order_host.py proves without a GPU that the cases reach the edges they are named for.  Everything compared is an
integer and compared exactly."""
import os

import numpy as np
import pytest

import tile_order_cases as cs
import tile_order_checks as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


@pytest.fixture(scope="module")
def ctx(dr, synth):          # synth first: the generated scenes exist before this process touches the GPU
    c = dr.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hf(dr, ctx, synth):
    """hf_small resident on the context: (product scene, oracle scene, settings)"""
    from oracle import orc
    path = os.path.join(synth["dir"], "hf_small.rts")
    ps = dr.Scene.load(path, "")
    ps.build_bvh()
    os_ = orc.Scene(path, None)
    os_.build_bvh()
    ctx.upload(ps)
    return ps, os_, ps.settings()


class options:
    """set the given options, put back what they were"""

    def __init__(self, ctx, **opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        self.before = {k: self.ctx.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.before.items():
            self.ctx.set_option(k, v)


def compared_words(words, regions):
    """the words of region_start the persistent kernel reads"""
    return words[:regions + 1].tolist() + words[tc.MAX_REGIONS + 1:tc.MAX_REGIONS + 1 + regions].tolist()


@pytest.mark.parametrize("name", [c.name for c in cs.CASES])
def test_known_answer(ctx, name):
    """tile_cost element for element; order, starts and counts through the comparison; twice, with equal normalised results"""
    c = cs.BY_NAME[name]
    cost = c.cost()
    pix = cs.pixels(cost)
    ref = c.reference(cost)
    runs = []
    for _ in range(2):
        got_cost, order, words = ctx.kat_tile_feedback(pix, c.regions, c.heavy_factor, c.split_steps, c.split_limit)
        assert np.array_equal(got_cost, cost), "tile_cost differs first at tile %d" % int(np.flatnonzero(got_cost != cost)[0])
        difference = tc.first_difference(ref, order, words)
        assert difference is None, difference
        runs.append((ref.normalised(order).tolist(), compared_words(words, c.regions)))
    assert runs[0] == runs[1]


@pytest.mark.parametrize("ntiles", cs.TILE_COST_COUNTS)
def test_tile_cost_takes_the_maximum_at_any_lane(ctx, ntiles):
    """tile counts that are no multiple of the four tiles a block takes; costs over the whole uint32 range, the maximum at lane 0, 31, 32 or 63"""
    cost = cs.huge(ntiles, 1) if ntiles > 3 else np.array([7, 0, cs.U32_MAX][:ntiles], dtype=np.uint32)
    got, order, words = ctx.kat_tile_feedback(cs.pixels(cost), 1, 0, 0, 0)
    assert np.array_equal(got, cost)
    assert order.tolist() == list(range(ntiles)) and words[:2].tolist() == [0, ntiles] and words[tc.MAX_REGIONS + 1] == 0


def test_refusals(dr, ctx):
    pix = np.ones(600 * 64, dtype=np.uint32)
    for ntiles, regions, limit in ((0, 1, 0), (-1, 1, 0), (600, 0, 0), (600, 2, 0), (600, 4, 0), (600, 16, 0), (511, 8, 0), (64, 8, 0), (600, 1, -1), (600, 8, -1)):
        with pytest.raises(dr.DogerayError) as e:
            ctx.kat_tile_feedback(pix, regions, 1, 400, limit, ntiles=ntiles)
        assert e.value.code == dr.ERR_INVALID, (ntiles, regions, limit)
    got, order, words = ctx.kat_tile_feedback(pix[:512 * 64], 8, 1, 400, 0)              # the smallest eight-region launch is accepted
    assert tc.first_difference(tc.Reference(got, 8, 1, 400, 0), order, words) is None


def test_live_order_is_the_reference_of_the_recorded_costs(dr, ctx, hf):
    """960 tiles in eight regions with splitting: the order the context holds after two frames of one view is the reference's order of the
    per-pixel costs it recorded, both frames are the oracle's, and some region has tiles to split (otherwise the case would be vacuous)"""
    ps, os_, s = hf
    W, H = 320, 192
    st = dr.pack_settings13(s, 1, spp=1)
    want, _ = os_.render(st, W, H, s.background, 41, nthreads=4)
    with options(ctx, kernel=1, short_one_queue=0, feedback_every=1, batch_frames=1, split_parts=4, split_steps=16, split_waves=100):
        first = ctx.render_frame(st, W, H, s.background, 41)
        second = ctx.render_frame(st, W, H, s.background, 41)
        live = ctx.tile_order()
        pix = ctx.pixel_cost(W, H, raw=True)
    assert np.array_equal(first, want) and np.array_equal(second, want)
    assert live is not None and live["regions"] == 8 and live["ntiles"] == 960 and pix.shape == (960 * 64,)
    assert (live["heavy_factor"], live["split_steps"]) == (1, 16) and live["split_limit"] > 0
    ref = tc.Reference(tc.tile_cost(pix, 960), 8, live["heavy_factor"], live["split_steps"], live["split_limit"])
    difference = tc.first_difference(ref, live["order"], live["region_start"])
    assert difference is None, difference
    counts = live["region_start"][tc.MAX_REGIONS + 1:]
    print("live order: split counts %s of limit %d per region, %d heavy tiles" % (counts.tolist(), live["split_limit"] // 8, int(ref.heavy.sum())))
    assert counts.max() > 0


def test_pixels_where_a_wave_owns_several_groups(dr, ctx, hf):
    """1024 x 520 = 8320 tiles, eight regions, the work-sharing build with splitting: a launch without an order, one with the first order, one with
    the refreshed order and a batch of three frames, every pixel against the oracle"""
    ps, os_, s = hf
    W, H, stride = 1024, 520, 1000003
    st = dr.pack_settings13(s, 1, spp=1)
    want = [os_.render(st, W, H, s.background, 9 + k * stride, nthreads=min(16, os.cpu_count() or 4))[0].astype(np.int64) for k in range(3)]
    assert ctx.get_option("coop_tiles_per_wave") == 32 and ctx.get_option("split_parts") == 4
    with options(ctx, kernel=1, short_one_queue=0, split_steps=16):
        for what in ("no order", "first order", "refreshed order"):
            got = ctx.render_frame(st, W, H, s.background, 9)
            assert np.array_equal(got, want[0]), what
        live = ctx.tile_order()
        ctx.accum_reset(W, H)
        ctx.render_accumulate(st, W, H, s.background, 9, stride, 3)
        acc = ctx.accum_read()
    assert np.array_equal(acc, want[0] + want[1] + want[2])
    assert live is not None and live["regions"] == 8 and live["ntiles"] == 8320
    assert live["region_start"][:9].tolist() == tc.region_bounds(8320, 8) and sorted(live["order"].tolist()) == list(range(8320))
    assert live["region_start"][tc.MAX_REGIONS + 1:].max() > 0


def test_pixel_cost_covers_the_whole_tiles_of_any_frame_size(dr, ctx, hf):
    ps, os_, s = hf
    st = dr.pack_settings13(s, 1, spp=1)
    with options(ctx, kernel=1):
        ctx.render_frame(st, 100, 75, s.background, 3)
        cost = ctx.pixel_cost(100, 75)
        flat = ctx.pixel_cost(100, 75, raw=True)
    assert cost.shape == (96, 72) and cost.min() >= 1
    assert flat.shape == (12 * 9 * 64,) and np.array_equal(flat.reshape(12, 9, 8, 8).transpose(0, 2, 1, 3).reshape(96, 72), cost)
