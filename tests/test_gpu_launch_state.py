"""What a render launch caches per view -- the tile order, the camera rays' tile words (certificate and entry table), the sky split
(dogeray_amd/csrc/launch_state.hpp) -- through one scripted walk of ONE context over the transitions the other tests visit one
at a time: tests/launch_state_walk.py lists the steps.  hf_small and city_small, frames of 64 x 64 and 128 x 64: two tile grids, both below the 512
tiles at which eight queues start -- none of the rules depends on the size.  The oracle's frames are rendered before the process touches the GPU.

After every step the accumulator equals the sum of the oracle's frames byte for byte, and the read-backs answer what the step implies: camera_entry()
the host build's table of the resident scene and the view (as tests/test_gpu_camera_entry.py computes it) or nothing, cert_levels() present or absent,
sky_tiles() the table's count of ENTRY_NONE words and the rest, or 0 / 0 for a launch that was not split, tile_order() the last feedback's argument
block and the order's length.

Step 3 (first sight of a single-frame view) computes no table and its launch reads none; dr_stats_camera_entry goes on answering the last table that
was computed, view A's, until step 4 computes B's -- that is what the skip has always left behind, and what is pinned here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_state_walk as walk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


@pytest.fixture(scope="module")
def walked(dr, synth):
    world = walk.prepare(dr, synth)          # first: the oracle has rendered before this process touches the GPU
    ctx = dr.Context(0)
    try:
        return list(walk.steps(ctx, world))
    finally:
        ctx.close()


def test_the_walk_has_every_step(walked):
    assert [s["label"].split()[0] for s in walked] == ["1", "2", "3", "4", "5", "5", "6", "6", "7", "7", "7", "8", "8", "9", "9", "10", "11", "12", "13"]


def test_accumulators_equal_the_oracles_sums(walked):
    for s in walked:
        differ = int((s["acc"] != s["want_acc"]).any(axis=2).sum()) if s["acc"].shape == s["want_acc"].shape else -1
        print("%-36s %d pixels differ" % (s["label"], differ))
        assert differ == 0, s["label"]


def test_read_backs_answer_what_the_step_implies(walked):
    for s in walked:
        print("%-36s entry %s levels %d sky %s order %s" % (s["label"], None if s["entry"] is None else len(s["entry"]), s["levels"], s["sky"], s["order"]))
        if s["want_entry"] is None:
            assert s["entry"] is None, s["label"]
        else:
            assert s["entry"] is not None and np.array_equal(s["entry"], s["want_entry"]), s["label"]
        assert s["levels"] == s["want_levels"], s["label"]
        assert tuple(s["sky"]) == tuple(s["want_sky"]), (s["label"], s["sky"], s["want_sky"])
        assert s["order"] == s["want_order"], (s["label"], s["order"], s["want_order"])
    # the walk is no walk over nothing: tiles were left to the sky, and tables differed from step to step
    assert any(s["sky"][0] > 0 for s in walked) and len({s["entry"].tobytes() for s in walked if s["entry"] is not None}) >= 5
