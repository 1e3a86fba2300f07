"""The persistent kernel's queue cursors on the GPU (launch_plan.hpp cursor_take; options queue_cursor_stride, queue_cursor_skew): a
launch's cursors lie `stride` words apart in its block of the context's ring, a 128-byte line each with the default stride.  Which wave claims which
unit enters no arithmetic, so every layout must give the same bytes.

The suite's small height field (hf_small) at 64 x 64 -- 64 tiles, one queue -- and at 256 x 128 -- 512 tiles, the smallest frame that gets a queue
per XCD (launch_plan.hpp plan_regions; coop_tiles_per_wave 0, so that no launch counts as short and falls back to one queue).  The lean builds are
forced as tests/test_gpu_step_control.py forces them: coop_steps 0, occupancy 6 and 5.

  * 1, 8 and 32 frames per launch, packed cursors (stride 1) and the default stride, six and five waves per SIMD: every accumulator against the
    oracle's bytes and against the packed launch's.
  * Every stride on offer, and a skewed block, at 256 x 128: the same bytes.
  * A fresh context taken across the ring's wrap by launches of one 64 x 64 frame, three more than the ring has blocks, for the default stride, the
    packed one and the widest: the accumulator against the oracle's sum and against the sum of the same frames rendered one by one.
  * The pipeline across the wrap: groups of eight frames with the widest stride (a ring of seven blocks), and one frame per launch, two launches side
    by side, with the default stride -- the launch that clears the ring runs alone (pipeline_state.hpp group_plan), and the sums are the oracle's.

The oracle's frames are rendered once per size and shared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

pytestmark = pytest.mark.gpu

SMALL, WIDE = (64, 64), (256, 128)
SEED, STRIDE = 41, 1000003
BATCHES = (1, 8, 32)
PACKED = 1
GROUPS = 10                        # pipelined groups of eight at the widest stride: the ring's seven blocks and three more


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


@pytest.fixture(scope="module")
def world(dr, hk, synth):          # synth first: the scene exists, and the oracle has rendered, before this process touches the GPU
    from oracle import orc
    lay = hk.cursor_layout()
    path = os.path.join(synth["dir"], "hf_small.rts")
    o = orc.Scene(path, None); o.build_bvh()
    sc = dr.Scene.load(path, ""); sc.build_bvh()
    s = sc.settings()
    st = dr.pack_settings13(s, 1, spp=1, depth=10)
    across = lay["ring_launches"] + 3
    w = {"scene": sc, "st": st, "bg": s.background, "lay": lay, "across": across, "oracle": {}}
    for (W, H), n, at in ((SMALL, max(across, 8 * GROUPS), BATCHES + (GROUPS, 8 * GROUPS, across)), (WIDE, max(BATCHES), BATCHES)):
        total, sums = np.zeros((W, H, 3), np.int64), {}
        for k in range(n):
            total += o.render(st, W, H, s.background, SEED + STRIDE * k, nthreads=8)[0]
            if k + 1 in at:
                sums[k + 1] = total.copy(); sums[k + 1].flags.writeable = False
        w["oracle"][(W, H)] = sums
    o.close()
    return w


def _context(dr, world, **options):
    c = dr.Context(0)
    c.upload(world["scene"])
    for name, value in dict({"coop_steps": 0, "coop_tiles_per_wave": 0}, **options).items():
        c.set_option(name, value)
    return c


@pytest.fixture(scope="module")
def ctx(dr, world):
    c = _context(dr, world)
    assert c.get_option("queue_cursor_stride") == world["lay"]["stride"] and c.get_option("queue_cursor_skew") == 0
    yield c
    c.close()


def _launch(c, world, size, occ, frames, stride, skew=0):
    """one launch of `frames` frames by the lean build of `occ` waves per SIMD with this cursor layout: the accumulator"""
    W, H = size
    c.set_option("occupancy", occ)
    c.set_option("batch_frames", frames)
    c.set_option("queue_cursor_stride", stride)
    c.set_option("queue_cursor_skew", skew)
    c.stats_reset()
    c.accum_reset(W, H)
    c.render_accumulate(world["st"], W, H, world["bg"], SEED, STRIDE, frames)
    assert c.stats()["launches"] == 1
    return c.accum_read().astype(np.int64)


def _differ(a, b):
    return "%d pixels differ" % int((a != b).any(axis=2).sum())


def test_the_two_sizes_get_one_queue_and_eight(hk):
    for frames in BATCHES:
        assert hk.plan_regions(SMALL[0] // 8 * (SMALL[1] // 8), frames, 1, 1, 0, 256) == 1
        assert hk.plan_regions(WIDE[0] // 8 * (WIDE[1] // 8), frames, 1, 1, 0, 256) == 8
    assert hk.plan_regions(WIDE[0] // 8 * (WIDE[1] // 8) - 1, 32, 1, 1, 0, 256) == 1      # the smallest frame that does


@pytest.mark.parametrize("occ", [6, 5])
@pytest.mark.parametrize("size", [SMALL, WIDE])
def test_packed_and_strided_cursors_equal_the_oracle(hk, world, ctx, size, occ):
    tiles = size[0] // 8 * (size[1] // 8)
    for frames in BATCHES:
        cfg = {"traversal": 2, "occupancy": occ, "schedule": 0, "num_cus": 256, "coop_tiles_per_wave": 0, "count": 0}
        b = dict(zip(hk.BUILD_FIELDS, hk.persistent_plan(cfg, tiles * frames, 0, 0, 0)))
        assert (b["occ"], b["wide"], b["coop"], b["count"], b["perframe"]) == (occ, 1, 0, 0, 0), b
        want = world["oracle"][size][frames]
        packed = _launch(ctx, world, size, occ, frames, PACKED)
        strided = _launch(ctx, world, size, occ, frames, world["lay"]["stride"])
        assert want.any()
        assert np.array_equal(packed, want), "%s, %d frames, %d waves, packed against the oracle: %s" % (size, frames, occ, _differ(packed, want))
        assert np.array_equal(strided, want), "%s, %d frames, %d waves, strided against the oracle: %s" % (size, frames, occ, _differ(strided, want))
        assert np.array_equal(strided, packed), "%s, %d frames, %d waves, strided against packed: %s" % (size, frames, occ, _differ(strided, packed))


def test_every_stride_on_offer_and_a_skewed_block(world, ctx):
    want = world["oracle"][WIDE][8]
    for stride, skew in ((16, 0), (64, 0), (1024, 0), (1024, 31), (1, 12), (1, 25), (world["lay"]["stride"], 5), (7, 0), (7, 3)):
        got = _launch(ctx, world, WIDE, 6, 8, stride, skew)
        assert np.array_equal(got, want), "stride %d, skew %d: %s" % (stride, skew, _differ(got, want))


@pytest.mark.parametrize("which", ["default", "packed", "widest"])
def test_a_context_across_the_ring_s_wrap(dr, hk, world, which):
    """a launch whose block no longer fits clears the ring first: a cursor that kept an earlier launch's count would hand out no unit, or too few"""
    W, H = SMALL
    stride = {"default": world["lay"]["stride"], "packed": PACKED, "widest": world["lay"]["stride_max"]}[which]
    n = hk.cursor_ring_blocks(stride) + 3
    assert n in (GROUPS, world["across"])
    c = _context(dr, world, queue_cursor_stride=stride, batch_frames=1)
    try:
        c.stats_reset()
        c.accum_reset(W, H)
        for k in range(n):
            c.render_accumulate(world["st"], W, H, world["bg"], SEED + STRIDE * k, STRIDE, 1)
        assert c.stats()["launches"] == n
        got = c.accum_read().astype(np.int64)
        singles = np.zeros((W, H, 3), np.int64)
        for k in range(n):                                  # (these cross the wrap a second time)
            singles += c.render_frame(world["st"], W, H, world["bg"], SEED + STRIDE * k)
    finally:
        c.close()
    want = world["oracle"][SMALL][n]
    assert np.array_equal(got, singles), "%d launches against the sum of single frames: %s" % (n, _differ(got, singles))
    assert np.array_equal(got, want), "%d launches against the oracle's sum: %s" % (n, _differ(got, want))


@pytest.mark.parametrize("group, which", [(8, "widest"), (1, "default")])
def test_the_pipeline_across_the_wrap(dr, hk, world, group, which):
    """the group that meets the wrap clears the ring on its own stream and runs alone; the frames' sum is the oracle's"""
    W, H = SMALL
    stride = {"default": world["lay"]["stride"], "widest": world["lay"]["stride_max"]}[which]
    launches = hk.cursor_ring_blocks(stride) + 3
    frames = launches * group
    assert frames in world["oracle"][SMALL], frames
    c = _context(dr, world, queue_cursor_stride=stride, pipe_group=group)
    try:
        c.stats_reset()
        c.accum_reset(W, H)
        c.render_accumulate_pipelined(world["st"], W, H, world["bg"], SEED, STRIDE, frames)
        s = c.stats()
        got = c.accum_read().astype(np.int64)
    finally:
        c.close()
    assert (s["frames"], s["launches"]) == (frames, launches), s
    want = world["oracle"][SMALL][frames]
    assert np.array_equal(got, want), "%d frames in groups of %d: %s" % (frames, group, _differ(got, want))
