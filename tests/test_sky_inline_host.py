"""Sky tiles rendered by the persistent kernel's retiring waves (option sky_tiles = 2), on the host build of the kernel's own code
(tools/host_kernel.cpp):
 * launch_plan.hpp's unit map -- unit number -> (position in the sky list, first frame, frames) -- covers every (sky tile, frame) of a launch exactly
   once, for every batch, chunk and list length, a last short chunk and a batch below the chunk among them;
 * device_sky.hpp sky_tile_frames, the body the sky kernel and the retiring waves share, summed over a tile's units in any order, equals sky_pixel
   summed over the launch's frames, int for int, and writes the cost words of the sky tiles' pixels only.
No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tools"))
import camera_entry_cases as cases
from camera_entry_cases import SEED, SIZES, STRIDE

CHUNKS = (1, 3, 8, 0)      # 0: the launch's whole batch


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    return dogeray_amd


@pytest.mark.parametrize("chunk", CHUNKS)
def test_units_cover_every_tile_and_frame_once(chunk):
    import host_kernel
    for batch in range(1, 34):
        frames = chunk if 0 < chunk < batch else batch                     # frames per unit
        chunks = -(-batch // frames)
        for n_sky in (0, 1, 7):
            n = host_kernel.sky_units(n_sky, batch, chunk)
            assert n == n_sky * chunks, (batch, chunk, n_sky)
            seen = np.zeros((n_sky, batch), np.int32)
            for u in range(n):
                index, first, count = host_kernel.sky_unit(u, batch, chunk)
                assert 0 <= index < n_sky and first % frames == 0 and 1 <= count <= frames and first + count <= batch, (batch, chunk, n_sky, u)
                assert count == frames or first + count == batch           # only a tile's last chunk is short
                seen[index, first:first + count] += 1
            assert (seen == 1).all(), (batch, chunk, n_sky)
    # more frames per unit than the batch has: the whole batch
    assert host_kernel.sky_units(7, 5, 8) == 7 and host_kernel.sky_unit(6, 5, 8) == (6, 0, 5)
    assert host_kernel.sky_units(7, 33, 8) == 35 and host_kernel.sky_unit(34, 33, 8) == (6, 32, 1)


@pytest.mark.parametrize("size", SIZES)
def test_units_of_a_tile_sum_to_its_sky_pixels(dr, synth, tmp_path_factory, size):
    import host_kernel
    W, H = size
    path, tex = cases.paths(synth, tmp_path_factory.mktemp("skyinline"))["hf_1"]
    hs = host_kernel.Scene(path, tex)
    s = dr.Scene.load(path, tex).settings()
    rng = np.random.default_rng(W)
    for spp in (1, 2):
        st = cases.views("hf_1", dr.pack_settings13(s, 1, spp=spp))[0]     # hf_small's own view
        codes = hs.camera_entry(st, W, H)[0]
        tiles = np.nonzero(codes == -1)[0].astype(np.int32)
        assert 0 < len(tiles) < len(codes)
        gy = H // 8
        lane = np.arange(64)
        xs = ((tiles // gy)[:, None] * 8 + (lane >> 3)[None, :]).ravel()
        ys = ((tiles % gy)[:, None] * 8 + (lane & 7)[None, :]).ravel()
        for batch in (1, 3, 9):
            want = np.zeros((W, H, 3), np.int64)
            want[xs, ys] = hs.sky_pixel(st, W, H, s.background, SEED, STRIDE, batch, xs, ys)
            assert want.any() == (s.background > 0)
            for chunk in CHUNKS:
                n = host_kernel.sky_units(len(tiles), batch, chunk)
                for perm in (None, rng.permutation(n)):
                    cost = np.full(len(codes) * 64, 0xdead, np.uint32)
                    acc, ran = hs.sky_units_render(st, W, H, s.background, SEED, STRIDE, batch, chunk, tiles, perm=perm, cost=cost)
                    assert ran == n
                    assert np.array_equal(acc.astype(np.int64), want), (spp, batch, chunk)
                    sky = np.repeat(codes == -1, 64)
                    assert (cost[sky] == 0).all() and (cost[~sky] == 0xdead).all(), (spp, batch, chunk)
