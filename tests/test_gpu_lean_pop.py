"""The lean six-wave build's pop (dogeray_amd/csrc/device_wide.hpp wide_pop_lean) on the GPU, on small frames where a pop can go wrong.
The six-wave lean build is forced as tests/test_gpu_sample_order.py forces it (no work sharing: coop_steps 0; occupancy 6); with occupancy 5 the same
options give the five-wave lean build, which keeps wide_pop.  Scenes, each at 64 x 64, depth 10:

  * nothing in view: two triangles behind the camera (no entry table for such a view: the camera rays start at the root) -- the root's test
    enters no child and the first pop finds the stack empty;
  * two and five triangles: unused child slots in the root, leaves right under it -- the stack is empty at the first pops;
  * a chain of shrinking triangles whose tree is at least as deep as the deepest of the suite's scenes: the stack is filled and emptied;
  * golden/scenes/lots.rts: spheres beside triangles.

(An empty scene and a scene of one triangle, which the issue names too, cannot be built: the library and the oracle both refuse a scene of fewer
than two objects, as the reference recurses without bound there.  The test asserts the refusal.)

Per scene one frame per launch, and a launch of 8 frames with sample_order 1, are compared byte for byte with the oracle and with the five-wave
lean build; for the one-frame launches dr_stats_pixel_cost -- the node and leaf steps of every pixel -- must be equal pixel for pixel between the
two builds: equal steps pin the traversal order, not only its result.  The oracle's frames are rendered once per scene and shared."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
from conftest import SCENES, with_settings
import ray_cases

pytestmark = pytest.mark.gpu

W, H = 64, 64
TILES = (W // 8) * (H // 8)
SEED, STRIDE = 29, 1000003
FRAMES = 8
HEADER = "*,0.5,-3.0,2.0,0.01,0,0,0,4,45,10,1,1,no,64,64"      # depth 10
NAMES = ("nothing", "two", "five", "deep", "lots")
RESTORE = (("occupancy", 6), ("coop_steps", 2), ("sample_order", 1), ("batch_frames", 32))


def _tris(n):
    """n triangles around the origin, in view, with gaps between them"""
    return [ray_cases.tri_line((-1.0 + 0.45 * k, 0.1 * k, -0.3), (-0.7 + 0.45 * k, 0.1 * k, -0.2), (-0.9 + 0.45 * k, 0.1 * k + 0.05, 0.4), k % 3) for k in range(n)]


def _chain(n=30, per=3, ratio=0.6):
    """clusters of `per` triangles, each cluster `ratio` times the size of the one before and as much nearer to the origin: the builder peels them
    off one by one, a tree far deeper than a balanced one of 90 leaves"""
    lines = []
    for k in range(n):
        s = ratio ** k
        for i in range(per):
            x = 1.5 * s + 0.1 * s * i
            lines.append(ray_cases.tri_line((x, 0.0, 0.0), (x + 0.05 * s, 0.0, 0.3 * s), (x, 0.2 * s, 0.05 * s), i % 3))
    return lines


def _write(path, lines):
    with open(path, "w") as f:
        f.write("\n".join([HEADER] + lines) + "\n")
    return path


@pytest.fixture(scope="module")
def paths(tmp_path_factory, synth):
    d = str(tmp_path_factory.mktemp("lean_pop"))
    behind = [ray_cases.tri_line((1.0, -6.0, 4.0), (1.3, -6.0, 4.1), (1.1, -6.2, 4.5)), ray_cases.tri_line((1.5, -6.5, 4.0), (1.8, -6.5, 4.1), (1.6, -6.7, 4.5))]
    return {"dir": d, "nothing": _write(os.path.join(d, "nothing.rts"), behind), "two": _write(os.path.join(d, "two.rts"), _tris(2)),
            "five": _write(os.path.join(d, "five.rts"), _tris(5)), "deep": _write(os.path.join(d, "deep.rts"), _chain()),
            "lots": with_settings(os.path.join(SCENES, "lots.rts"), os.path.join(d, "lots.rts"), HEADER),
            "suite": [os.path.join(synth["dir"], n) for n in ("hf_small.rts", "bunny_small.rts", "city_small.rts", "matball.rts")]}


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


@pytest.fixture(scope="module")
def world(dr, paths):          # paths first: the scenes exist, and the oracle has rendered, before this process touches the GPU
    from oracle import orc
    w = {}
    for name in NAMES:
        o = orc.Scene(paths[name], None); o.build_bvh()
        sc = dr.Scene.load(paths[name], ""); sc.build_bvh()
        s = sc.settings()
        st = dr.pack_settings13(s, 1, spp=1)
        frames = [o.render(st, W, H, s.background, SEED + STRIDE * k, nthreads=8)[0].astype(np.int64) for k in range(FRAMES)]
        for f in frames: f.flags.writeable = False
        w[name] = {"scene": sc, "st": st, "bg": s.background, "oracle": frames}
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


def test_fewer_than_two_objects_are_refused(paths):
    """the issue's empty scene and its scene of one triangle: neither side builds them"""
    import dogeray_amd as dr
    from oracle import orc
    for name, lines in (("none", []), ("one", _tris(1))):
        p = _write(os.path.join(paths["dir"], name + ".rts"), lines)
        with pytest.raises(Exception, match="at least 2 objects"):
            sc = dr.Scene.load(p, ""); sc.build_bvh()
        with pytest.raises(Exception, match="at least 2 objects"):
            o = orc.Scene(p, None); o.build_bvh()


def test_the_deep_scene_is_as_deep_as_the_suites_deepest(paths):
    import host_kernel
    depth = lambda p, tex="": host_kernel.Scene(p, tex).wide_info(2)["wide_depth"]
    deep = depth(paths["deep"])
    others = [depth(p) for p in paths["suite"]] + [depth(os.path.join(SCENES, f), os.path.join(SCENES, "..", "textures")) for f in sorted(os.listdir(SCENES))
                                                   if f.endswith(".rts")]
    assert deep >= max(others) and deep > 8, (deep, others)
    assert depth(paths["two"]) == 1 and depth(paths["five"]) == 2, "the root is not alone in `two`, or `five` has more than two levels"


@pytest.mark.parametrize("name", NAMES)
def test_six_waves_equal_the_oracle_and_five_waves(world, ctx, name):
    e = world[name]
    ctx.upload(e["scene"])
    if name == "deep":
        assert ctx.get_option("wide_depth") > 8
    for frames in (FRAMES, 1):      # (the launch of several frames first: the view's entry table exists from then on)
        want = sum(e["oracle"][:frames])
        six, cost6 = _launch(ctx, e, 6, frames)
        five, cost5 = _launch(ctx, e, 5, frames)
        assert np.array_equal(six, want), "%s, %d frames, six waves against the oracle: %d pixels differ" % (name, frames, int((six != want).any(axis=2).sum()))
        assert np.array_equal(five, want), "%s, %d frames, five waves against the oracle: %d pixels differ" % (name, frames, int((five != want).any(axis=2).sum()))
        if frames == 1:
            assert len(cost6) == TILES * 64
            assert np.array_equal(cost6, cost5), "%s: the steps of %d pixels differ between the builds" % (name, int((cost6 != cost5).sum()))
            if name == "nothing":
                codes = ctx.camera_entry()
                assert len(codes) == TILES and (cost6 <= 1).all(), "a camera ray took more than the root's step"
            else:
                assert cost6.any() and len(np.unique(want.reshape(-1, 3), axis=0)) > 8, "the scene is not in view"
