"""Sky tiles (option sky_tiles) on the host build of the kernel's own code (tools/host_kernel.cpp):
 * hk_sky_split, the partition of a launch's tile order into the geometry tiles the persistent kernel keeps and the sky tiles (device_sky.hpp
   SkyKeep, device_split.hpp order_split_plain), against the stable partition written in numpy (tests/split_cases.py);
 * hk_sky_pixel, the per-pixel body of sky_tiles_kernel (device_sky.hpp sky_pixel), against the host kernel's own render of the same pixels from the
   root, int for int, for every tile the views' entry tables give the code ENTRY_NONE;
 * the launch plan's decision: only the lean build of the wide walk that adds a batch into one buffer is split.
No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tools"))
import camera_entry_cases as cases
import split_cases as sp
from camera_entry_cases import SEED, SIZES, STRIDE

SKY_NAMES = ("hf_1", "hf_0.1", "cube", "tiny_2", "grid_small", "matball")


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    return dogeray_amd


@pytest.fixture(scope="module")
def paths(synth, tmp_path_factory):
    return cases.paths(synth, tmp_path_factory.mktemp("skyhost"))


@pytest.mark.parametrize("regions,tiles", [(1, 40), (8, 512), (1, 512), (8, 40)])
def test_split_is_a_stable_partition(regions, tiles):
    import host_kernel
    rng = np.random.default_rng(100 * regions + tiles)
    cases_run = 0
    for c in sp.cases(rng, regions, tiles):
        kind, identity, order, rs, sky = c.kind, c.identity, c.order, c.rs, ~c.kept      # (a "region" case: one whole region sky)
        word = sp.words(rng, c.kept)
        lo, lrs, sl = host_kernel.sky_split(order, c.rs_in(), word, regions)
        want_lo, want_lrs, want_sl = sp.partition(order, rs, ~sky, regions)
        assert np.array_equal(lo, want_lo), (kind, identity)
        assert np.array_equal(lrs, want_lrs), (kind, identity, lrs, want_lrs)
        assert np.array_equal(sl, want_sl), (kind, identity)
        assert np.array_equal(sl, np.nonzero(sky)[0]), (kind, identity)
        assert np.array_equal(np.sort(np.concatenate([lo, sl])), np.arange(tiles)), (kind, identity)
        assert lrs[regions] == len(lo) and not lrs[sp.MAX_REGIONS + 1:].any()
        cases_run += 1
    assert cases_run == 12


def test_sky_pixels_equal_the_render_from_the_root(dr, paths):
    import host_kernel
    frames = 2
    total = {}
    for name in SKY_NAMES:
        path, tex = paths[name]
        hs = host_kernel.Scene(path, tex)
        s = dr.Scene.load(path, tex).settings()
        for spp in (1, 2):
            st0 = dr.pack_settings13(s, 1, spp=spp)
            for st in (cases.lens(v, k) for v in cases.views(name, st0) for k in range(3)):
                for W, H in SIZES:
                    table = hs.camera_entry(st, W, H)
                    if table is None:
                        continue                       # (a lens too wide for its focus plane: the view gives no table and no launch is split)
                    codes = table[0]
                    tiles = np.nonzero(codes == -1)[0]
                    if spp == 1:
                        total[name] = total.get(name, 0) + len(tiles)
                    if len(tiles) == 0:
                        continue
                    gy = H // 8
                    lane = np.arange(64)
                    xs = ((tiles // gy)[:, None] * 8 + (lane >> 3)[None, :]).ravel()
                    ys = ((tiles % gy)[:, None] * 8 + (lane & 7)[None, :]).ravel()
                    got = hs.sky_pixel(st, W, H, s.background, SEED, STRIDE, frames, xs, ys)
                    want = sum(hs.render(st, W, H, s.background, SEED + STRIDE * f, traversal=2, nthreads=8, count=False)[0].astype(np.int64) for f in range(frames))
                    assert np.array_equal(got.astype(np.int64), want[xs, ys]), (name, spp, W, H)
    print("tiles without geometry over the views and sizes:", total)
    # (counted on the CPU when the test was written; the tables are tests/test_camera_entry_host.py's business)
    assert total == {"hf_1": 101, "hf_0.1": 62, "cube": 85, "tiny_2": 92, "grid_small": 183, "matball": 19}


def test_only_the_lean_build_is_split():
    import host_kernel
    cfg = {"traversal": 2, "occupancy": 6, "schedule": 0, "num_cus": 256, "coop_tiles_per_wave": 32, "count": 0}
    long_work, short_work = 32400 * 32, 32400

    def build(c, work, per_frame=0):
        return dict(zip(host_kernel.BUILD_FIELDS, host_kernel.persistent_plan(c, work, 2, per_frame, 0)))
    assert build(cfg, long_work)["coop"] == 0 and host_kernel.plan_sky_split(cfg, long_work, 2, 0, 0)                       # the bench's launch: lean, six waves
    assert host_kernel.plan_sky_split(dict(cfg, occupancy=5), long_work, 2, 0, 0)                                           # the five-wave lean build
    assert host_kernel.plan_sky_split(dict(cfg, coop_tiles_per_wave=0), 40 * 2, 2, 0, 0)                                    # the tests' launches
    assert build(dict(cfg, count=1), long_work)["count"] == 1 and not host_kernel.plan_sky_split(dict(cfg, count=1), long_work, 2, 0, 0)
    assert build(cfg, short_work)["coop"] == 1 and not host_kernel.plan_sky_split(cfg, short_work, 2, 0, 0)                 # one frame: work sharing
    assert build(cfg, long_work, 1)["perframe"] == 1 and not host_kernel.plan_sky_split(cfg, long_work, 2, 1, 0)            # a group's per-frame stores
    assert not host_kernel.plan_sky_split(dict(cfg, traversal=0), long_work, 2, 0, 0)                                       # the threaded walk


def test_option_and_call_are_documented(dr):
    root = os.path.join(HERE, "..")
    hdr = open(os.path.join(root, "include", "dogeray_amd.h")).read()
    src = open(os.path.join(root, "dogeray_amd", "csrc", "context.cpp")).read()
    assert '"sky_tiles"' in hdr and '"sky_tiles"' in src
    assert "int dr_stats_sky_tiles(dr_context* c, int* n_sky, int* n_geometry);" in hdr
    assert "dr_stats_sky_tiles" in dr.API_SYMBOLS and hasattr(dr.Context, "sky_tiles")
