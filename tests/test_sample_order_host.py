"""Which samples of a tile share a unit of the persistent kernel's queue (option sample_order; dogeray_amd/csrc/launch_plan.hpp tile_sample and
sample_order_magic, through tools/host_kernel.cpp: the functions the kernel's refill loop calls).  Sample j = 64 unit + slot of a tile, 0 <= j < 64 B,
is (pixel-in-tile p, frame f): order 0 (j % 64, j / 64), order 1 (j / B, j % B) with the division done by a multiply-high.  For both orders and every
B in 1 .. 256, exhaustively:

  * j -> (p, f) is a bijection of [0, 64 B) onto [0, 64) x [0, B);
  * the reciprocal form equals the plain / and %;
  * order 0 is today's (j % 64, j / 64), and B = 1 is the identity in both orders;
  * in order 1 a unit's samples are consecutive frames of at most ceil(64 / B) + 1 pixels."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

BATCHES = range(1, 257)


@pytest.fixture(scope="module")
def L():
    import host_kernel
    host_kernel.build()
    return host_kernel.lib()


@pytest.fixture(scope="module")
def samples(L):
    """(order, B) -> int32[64 B, 2]: every sample of a tile through the kernel's call, computed once"""
    out = {}
    for order in (0, 1):
        for B in BATCHES:
            a = np.full((64 * B, 2), -1, dtype=np.int32)
            L.hk_tile_samples(order, B, a.ctypes.data_as(C.POINTER(C.c_int)))
            a.flags.writeable = False
            out[(order, B)] = a
    return out


def test_the_word(L):
    """0 for order 0 and for one frame (ceil(2^32 / 1) does not fit a word), else ceil(2^32 / B); outside 1 .. 256 frames order 0"""
    for B in BATCHES:
        assert L.hk_sample_order_magic(0, B) == 0
        assert L.hk_sample_order_magic(1, B) == (0 if B == 1 else -(-2 ** 32 // B))
    for B in (0, -1, 257, 1 << 20):
        assert L.hk_sample_order_magic(1, B) == 0


@pytest.mark.parametrize("order", [0, 1])
def test_a_bijection_for_every_batch(samples, order):
    for B in BATCHES:
        a = samples[(order, B)]
        p, f = a[:, 0].astype(np.int64), a[:, 1].astype(np.int64)
        assert p.min() >= 0 and p.max() < 64 and f.min() >= 0 and f.max() < B, (order, B)
        assert len(np.unique(p * B + f)) == 64 * B, (order, B)


def test_the_reciprocal_is_the_division(samples):
    for B in BATCHES:
        j = np.arange(64 * B)
        a = samples[(1, B)]
        assert np.array_equal(a[:, 0], j // B) and np.array_equal(a[:, 1], j % B), B


def test_order_0_is_the_frame_major_one(samples):
    for B in BATCHES:
        j = np.arange(64 * B)
        a = samples[(0, B)]
        assert np.array_equal(a[:, 0], j % 64) and np.array_equal(a[:, 1], j // 64), B


def test_one_frame_is_the_identity(samples):
    j = np.arange(64)
    for order in (0, 1):
        a = samples[(order, 1)]
        assert np.array_equal(a[:, 0], j) and not a[:, 1].any(), order


def test_a_unit_is_consecutive_frames_of_few_pixels(samples):
    for B in BATCHES:
        a = samples[(1, B)].reshape(B, 64, 2)             # [unit, slot]
        most = -(-64 // B) + 1
        for u in range(B):
            p, f = a[u, :, 0], a[u, :, 1]
            assert len(np.unique(p)) <= most, (B, u)
            same = p[1:] == p[:-1]
            assert np.all(f[1:][same] == f[:-1][same] + 1), (B, u)                                  # a pixel's frames in a row
            assert np.all(p[1:][~same] == p[:-1][~same] + 1) and not f[1:][~same].any(), (B, u)   # ... then the next pixel from its frame 0
            assert np.all(f[:-1][~same] == B - 1), (B, u)


def test_the_single_call_is_the_same_function(L, samples):
    out = (C.c_int * 2)()
    for order, B in ((0, 1), (1, 1), (0, 20), (1, 20), (1, 3), (1, 255), (1, 256)):
        magic = L.hk_sample_order_magic(order, B)
        for j in (0, 1, 63, 64 * B - 1, (64 * B) // 2):
            L.hk_tile_sample(magic, B, j, out)
            assert (out[0], out[1]) == tuple(samples[(order, B)][j]), (order, B, j)


def test_the_option_is_documented(L):
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    hdr = open(os.path.join(root, "include", "dogeray_amd.h")).read()
    src = open(os.path.join(root, "dogeray_amd", "csrc", "context.cpp")).read()
    assert '"sample_order"' in hdr and '"sample_order"' in src
