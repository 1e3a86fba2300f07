"""The ring of the persistent kernel's queue cursors (dogeray_amd/csrc/launch_plan.hpp cursor_take, through tools/host_kernel.cpp: the one rule
context_render.cpp's enqueue_frame and context_pipeline.cpp's group plan both ask).  A launch's block is a cursor per tile queue,
`stride` words apart, and the sky units' cursor in its last slot: 9 stride words.  For every stride on offer (1, 16, 32, 64, 1024, the default) and
the skews the measurements used, over several passes of the ring:

  * a block starts at a multiple of the stride (skew 0) -- with the default stride no two of its cursors share a 128-byte line --, or `skew` words
    into a 128-byte line;
  * the blocks of one pass never overlap and all lie inside the allocation;
  * a wrap is reported exactly when the next block would not fit into the ring, and the block of a wrapping launch starts the ring again;
  * a cursor left by another layout (an option changed) wraps unless the new blocks would line up, and never yields an overlapping block.

And what a claim from such a cursor stands for: unit u of a tile is the sample indices 64 u .. 64 u + 63, mapped by tile_sample; for every n <= 256 frames
and both sample orders every (pixel, frame) of the tile is handed out exactly once, whatever order the claims come in."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

STRIDES = (1, 16, 32, 64, 1024)
SKEWS = (0, 1, 10, 12, 25, 31)
PASSES = 3


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


def _pitch(lay, stride, skew):
    words = lay["slots"] * stride
    return words if skew == 0 else -(-(skew + words) // lay["line_words"]) * lay["line_words"]


def test_the_layout_s_constants(hk):
    lay = hk.cursor_layout()
    assert lay["slots"] == 9 and lay["line_words"] == 32                       # eight queues and the sky units' cursor; 128 bytes
    assert lay["stride"] in STRIDES and lay["stride"] % lay["line_words"] == 0   # the default: a line of its own for every cursor
    assert lay["stride_max"] == max(STRIDES)
    for stride in STRIDES:
        for skew in SKEWS:
            n = hk.cursor_ring_blocks(stride, skew)
            assert n == min(lay["ring_launches"], lay["alloc_words"] // _pitch(lay, stride, skew)) and n >= 2, (stride, skew)
    assert hk.cursor_ring_blocks(lay["stride"]) == lay["ring_launches"] == 128   # what DESIGN.md 4.3 writes down


@pytest.mark.parametrize("stride", STRIDES)
def test_the_ring_rule_over_several_wraps(hk, stride):
    lay = hk.cursor_layout()
    words = lay["slots"] * stride
    for skew in SKEWS:
        pitch, blocks = _pitch(lay, stride, skew), hk.cursor_ring_blocks(stride, skew)
        cursor, taken, wraps = 0, [], 0
        for k in range(PASSES * blocks + 3):
            block, nxt, wrap = hk.cursor_take(cursor, stride, skew)
            fits = cursor + pitch <= blocks * pitch
            assert wrap == (not fits), (stride, skew, k)            # exactly when the next block would not fit
            assert wrap == (k > 0 and k % blocks == 0), (stride, skew, k)
            if wrap:
                wraps += 1; taken = []                               # the ring is cleared: a new pass
                assert block == skew and nxt == pitch
            assert 0 <= block and block + words <= nxt <= lay["alloc_words"], (stride, skew, k)
            assert block + (lay["slots"] - 1) * stride < block + words   # the sky cursor, the last slot, is inside the block
            if skew == 0:
                assert block % stride == 0, (stride, k)
            else:
                assert block % lay["line_words"] == skew, (stride, skew, k)
            assert all(block >= b + words for b in taken[-1:]) and (not taken or block > taken[-1]), (stride, skew, k)   # ascending and disjoint
            taken.append(block)
            cursor = nxt
        assert wraps == PASSES


def test_a_line_per_cursor_with_the_default_stride(hk):
    lay = hk.cursor_layout()
    stride, cursor = lay["stride"], 0
    for _ in range(2 * lay["ring_launches"]):
        block, cursor, _ = hk.cursor_take(cursor, stride, 0)
        lines = [(block + slot * stride) // lay["line_words"] for slot in range(lay["slots"])]
        assert len(set(lines)) == lay["slots"]


def test_a_strided_block_does_not_depend_on_the_skew(hk):
    """with a stride of a line or more every cursor keeps a line of its own wherever the block starts"""
    lay = hk.cursor_layout()
    for stride in (32, 64, 1024):
        for skew in SKEWS:
            block, _, _ = hk.cursor_take(0, stride, skew)
            assert len({(block + slot * stride) // lay["line_words"] for slot in range(lay["slots"])}) == lay["slots"], (stride, skew)


def test_a_cursor_left_by_another_layout(hk):
    """the words from the cursor on are zero; a block may start there if it lines up with the new pitch, else the ring starts again"""
    lay = hk.cursor_layout()
    for old in STRIDES:
        for new in STRIDES:
            for skew in (0, 12):
                cursor = 0
                for _ in range(5):
                    _, cursor, _ = hk.cursor_take(cursor, old, 0)
                    block, nxt, wrap = hk.cursor_take(cursor, new, skew)
                    pitch = _pitch(lay, new, skew)
                    assert wrap == (cursor % pitch != 0 or cursor + pitch > hk.cursor_ring_blocks(new, skew) * pitch), (old, new, skew, cursor)
                    assert (block >= cursor or wrap) and nxt <= lay["alloc_words"], (old, new, skew, cursor)
    for bad in (-1, lay["alloc_words"], 1 << 30):
        assert hk.cursor_take(bad, lay["stride"], 0) == (0, lay["slots"] * lay["stride"], True)


@pytest.mark.parametrize("order", [0, 1])
def test_every_sample_of_a_tile_is_claimed_once(hk, order):
    """The claims of one tile in a launch of n frames, as the refill loop makes them: claim u of the tile's n (one add to the queue's cursor each) hands
    out the sample indices 64 u + l, l = 0 .. 63, and launch_plan.hpp tile_sample says which (pixel, frame) an index is.  For every n <= 256, with the
    claims taken in any order: every (pixel, frame) exactly once.  (A claim stands for one unit: larger claims are not built.)"""
    import ctypes as C
    import numpy as np
    L = hk.lib()
    rng = np.random.default_rng(5)
    out = (C.c_int * 2)()
    for n in range(1, 257):
        magic = L.hk_sample_order_magic(order, n)
        whole = np.empty((64 * n, 2), np.int32)
        L.hk_tile_samples(order, n, whole.ctypes.data_as(C.POINTER(C.c_int)))
        seen = np.zeros((64, n), np.int32)
        for u in rng.permutation(n):                      # which wave's add comes first is not the kernel's to say
            unit = whole[64 * u:64 * u + 64]
            assert unit[:, 0].min() >= 0 and unit[:, 0].max() < 64 and unit[:, 1].min() >= 0 and unit[:, 1].max() < n, (order, n, u)
            np.add.at(seen, (unit[:, 0], unit[:, 1]), 1)
        assert (seen == 1).all(), (order, n)
        for u, l in ((0, 0), (n - 1, 63), (n // 2, 17)):  # ... and the refill loop's own call, one sample at a time, is the same function
            L.hk_tile_sample(magic, n, 64 * u + l, out)
            assert (out[0], out[1]) == tuple(whole[64 * u + l]), (order, n, u, l)


def test_the_options_are_documented():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    hdr = open(os.path.join(root, "include", "dogeray_amd.h")).read()
    src = open(os.path.join(root, "dogeray_amd", "csrc", "context.cpp")).read()
    for name in ('"queue_cursor_stride"', '"queue_cursor_skew"'):
        assert name in hdr and name in src
