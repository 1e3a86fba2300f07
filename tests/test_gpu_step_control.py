"""The six-wave lean build's step control (dogeray_amd/csrc/kernels_render.hip step_by_masks, device_walk.hpp step_masks) on the GPU:
who steps is decided from wave masks on the scalar unit and reaches the lanes as exec masks.  The builds are forced as tests/test_gpu_lean_pop.py
forces them (no work sharing: coop_steps 0; occupancy 6 against 5): the five-wave lean build keeps the per-lane rule and is the reference inside the
library.  Every frame is 64 x 64 at depth 10.

Scenes: that file's `nothing` (only node lanes, one step each), `two` (leaves right under the root), `deep` (a deep stack) and `lots` (spheres beside
triangles), and the suite's hf_small (9 800 triangles) and matball (textured spheres).

  * One frame per launch: its 64 units are far fewer than the waves, so every wave finds the queue empty at its first fetch and drains from then on --
    the arm of the rule where leaf and node lanes step together.  Against the oracle's bytes and the five-wave build's; dr_stats_pixel_cost -- the
    steps of every pixel -- equal pixel for pixel between the builds.
  * 8 frames per launch with sample_order 1: the same comparisons.
  * batch_frames 256 (hf_small, matball): 16 384 units, more than the 6 144 waves of the six-wave build, so waves walk with a full queue -- the arm
    where fewer than 20 leaf lanes wait while node lanes step, and a leaf step is taken without the node lanes.  The accumulator byte for byte
    against the five-wave build's and against the oracle's sum of the same 256 frames.

The oracle's frames are rendered once per scene and shared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
from conftest import SCENES, with_settings
import ray_cases
from test_gpu_lean_pop import HEADER, _chain, _tris, _write

pytestmark = pytest.mark.gpu

W, H = 64, 64
TILES = (W // 8) * (H // 8)
SEED, STRIDE = 31, 1000003
FRAMES = 8
FULL_QUEUE = 256
SMALL = ("nothing", "two", "deep", "lots")
SUITE = ("hf_small", "matball")
RESTORE = (("occupancy", 6), ("coop_steps", 2), ("sample_order", 1), ("batch_frames", 32))


@pytest.fixture(scope="module")
def paths(tmp_path_factory, synth):
    d = str(tmp_path_factory.mktemp("step_control"))
    behind = [ray_cases.tri_line((1.0, -6.0, 4.0), (1.3, -6.0, 4.1), (1.1, -6.2, 4.5)), ray_cases.tri_line((1.5, -6.5, 4.0), (1.8, -6.5, 4.1), (1.6, -6.7, 4.5))]
    return {"dir": d, "nothing": (_write(os.path.join(d, "nothing.rts"), behind), ""), "two": (_write(os.path.join(d, "two.rts"), _tris(2)), ""),
            "deep": (_write(os.path.join(d, "deep.rts"), _chain()), ""),
            "lots": (with_settings(os.path.join(SCENES, "lots.rts"), os.path.join(d, "lots.rts"), HEADER), ""),
            "hf_small": (os.path.join(synth["dir"], "hf_small.rts"), ""), "matball": (os.path.join(synth["dir"], "matball.rts"), synth["tex"])}


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


@pytest.fixture(scope="module")
def world(dr, paths):          # paths first: the scenes exist, and the oracle has rendered, before this process touches the GPU
    from oracle import orc
    w = {}
    for name in SMALL + SUITE:
        path, tex = paths[name]
        o = orc.Scene(path, tex or None); o.build_bvh()
        sc = dr.Scene.load(path, tex); sc.build_bvh()
        s = sc.settings()
        st = dr.pack_settings13(s, 1, spp=1, depth=10)
        n = FULL_QUEUE if name in SUITE else FRAMES
        total, sums = np.zeros((H, W, 3), np.int64), {}
        for k in range(n):
            total += o.render(st, W, H, s.background, SEED + STRIDE * k, nthreads=8)[0]
            if k + 1 in (1, FRAMES, FULL_QUEUE):
                sums[k + 1] = total.copy(); sums[k + 1].flags.writeable = False
        w[name] = {"scene": sc, "st": st, "bg": s.background, "oracle": sums}
        o.close()
    c = dr.Context(0)
    w["ctx"] = c
    yield w
    c.close()


@pytest.fixture()
def ctx(world):
    c = world["ctx"]
    try:
        yield c
    finally:
        for name, value in RESTORE:
            c.set_option(name, value)


def _build(ctx, frames):
    import host_kernel
    cfg = {"traversal": 2, "occupancy": ctx.get_option("occupancy"), "schedule": ctx.get_option("schedule"), "num_cus": 256,
           "coop_tiles_per_wave": ctx.get_option("coop_tiles_per_wave"), "count": 0}
    return dict(zip(host_kernel.BUILD_FIELDS, host_kernel.persistent_plan(cfg, TILES * frames, ctx.get_option("coop_steps"), 0, 0)))


def _launch(ctx, e, occ, frames):
    """one launch of `frames` frames by the lean build of `occ` waves per SIMD: (accumulator, per-pixel cost)"""
    ctx.set_option("coop_steps", 0)
    ctx.set_option("occupancy", occ)
    ctx.set_option("sample_order", 1)
    ctx.set_option("batch_frames", frames)
    b = _build(ctx, frames)
    assert (b["occ"], b["wide"], b["coop"], b["count"], b["perframe"]) == (occ, 1, 0, 0, 0), b
    ctx.stats_reset()
    ctx.accum_reset(W, H)
    ctx.render_accumulate(e["st"], W, H, e["bg"], SEED, STRIDE, frames)
    assert ctx.stats()["launches"] == 1
    return ctx.accum_read().astype(np.int64), ctx.pixel_cost(W, H, raw=True).copy()


def test_fewer_than_two_objects_are_still_refused(paths):
    import dogeray_amd as dr
    for name, lines in (("none", []), ("one", _tris(1))):
        p = _write(os.path.join(paths["dir"], name + ".rts"), lines)
        with pytest.raises(Exception, match="at least 2 objects"):
            sc = dr.Scene.load(p, ""); sc.build_bvh()


@pytest.mark.parametrize("name", SMALL + SUITE)
def test_six_waves_equal_the_oracle_and_five_waves(world, ctx, name):
    e = world[name]
    ctx.upload(e["scene"])
    for frames in (FRAMES, 1):      # (the launch of several frames first: the view's entry table exists from then on)
        want = e["oracle"][frames]
        six, cost6 = _launch(ctx, e, 6, frames)
        five, cost5 = _launch(ctx, e, 5, frames)
        assert np.array_equal(six, want), "%s, %d frames, six waves against the oracle: %d pixels differ" % (name, frames, int((six != want).any(axis=2).sum()))
        assert np.array_equal(five, want), "%s, %d frames, five waves against the oracle: %d pixels differ" % (name, frames, int((five != want).any(axis=2).sum()))
        assert len(cost6) == TILES * 64
        assert np.array_equal(cost6, cost5), "%s, %d frames: the steps of %d pixels differ between the builds" % (name, frames, int((cost6 != cost5).sum()))
        if name == "nothing":
            assert (cost6 <= frames).all(), "a camera ray took more than the root's step"
        else:
            assert cost6.any() and len(np.unique(want.reshape(-1, 3), axis=0)) > 8, "the scene is not in view"


@pytest.mark.parametrize("name", SUITE)
def test_a_full_queue_equals_five_waves_and_the_oracle(world, ctx, name):
    e = world[name]
    ctx.upload(e["scene"])
    assert TILES * FULL_QUEUE > 256 * 4 * 6      # more units than the six-wave build has waves (256 CUs, 4 SIMDs)
    six, _ = _launch(ctx, e, 6, FULL_QUEUE)
    five, _ = _launch(ctx, e, 5, FULL_QUEUE)
    assert np.array_equal(six, five), "%s: %d pixels differ between the builds" % (name, int((six != five).any(axis=2).sum()))
    want = e["oracle"][FULL_QUEUE]
    assert np.array_equal(six, want), "%s: %d pixels differ from the oracle's sum of %d frames" % (name, int((six != want).any(axis=2).sum()), FULL_QUEUE)
