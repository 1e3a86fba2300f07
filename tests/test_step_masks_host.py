"""Who takes a step of the wide walk (dogeray_amd/csrc/device_walk.hpp step_masks: the six-wave lean build's decision as a function of wave masks;
DESIGN.md 4.3) against the rule as render_persistent_kernel writes it per lane, through tools/host_kernel.cpp: the same header compiled for the host.

The rule, for one wave.  A lane walks when its word is a record's link (>= 0) and stands at a leaf when that link is odd; LANE_DONE (-1), LANE_REFILL (-2)
and LANE_RETIRED (-3) walk nowhere, whatever their low bit.  With leaves / nodes the counts of lanes at a leaf / at a node:

    do_leaves = leaves > 0 and (leaves >= leaf_min or nodes == 0 or draining)
    do_nodes  = not exclusive or not do_leaves or draining
    a lane steps      when it walks and (do_leaves if it is at a leaf else do_nodes)
    ... as a leaf     when it steps and is at a leaf

Cases: 0, 1, 19, 20, 21, 63 and 64 lanes at leaves, each with no, one and many node lanes (as many as fit), the rest of the wave in the three
non-walking states; draining and exclusive on and off; thresholds 1 and 20; the lanes of every case in several shuffled orders; and some thousands of
random waves.  The masks must be equal bit for bit.  No GPU.

What this does not run: the device's spellings of the count and of the lane's bit of a mask (device_prims.hpp wave_count, lane_bit: an s_bcnt1_i32_b64
and the inverse ballot; the host's are a popcount and bit 0).  tests/test_gpu_step_control.py runs those, pixel for pixel against the build that keeps
the per-lane rule."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

LANE_DONE, LANE_REFILL, LANE_RETIRED = -1, -2, -3
IDLE = (LANE_DONE, LANE_REFILL, LANE_RETIRED)
LEAF_COUNTS = (0, 1, 19, 20, 21, 63, 64)
THRESHOLDS = (1, 20)
SHUFFLES = 4
RANDOM_WAVES = 4000


def _wave(rng, n_leaf, n_node, shuffle):
    """64 lane words: n_leaf odd links, n_node even links (link 0, the root, among them), the rest cycling through the non-walking states"""
    leaf = 2 * rng.integers(0, 1 << 24, n_leaf) + 1
    node = 2 * rng.integers(0, 1 << 24, n_node)
    if n_node:
        node[0] = 0
    idle = np.array([IDLE[k % 3] for k in range(64 - n_leaf - n_node)], np.int64)
    w = np.concatenate([leaf, node, idle]).astype(np.int32)
    return rng.permutation(w) if shuffle else w


@pytest.fixture(scope="module")
def cases():
    """(node int32[n, 64], draining, leaf_min, exclusive int32[n]) and the (leaf count, node count) of the structured cases"""
    rng = np.random.default_rng(20)
    waves, counts = [], []
    for n_leaf in LEAF_COUNTS:
        for n_node in sorted({0, 1, 64 - n_leaf} & set(range(0, 64 - n_leaf + 1))) + ([(64 - n_leaf) // 2] if 64 - n_leaf >= 4 else []):
            for s in range(SHUFFLES):
                waves.append(_wave(rng, n_leaf, n_node, s > 0)); counts.append((n_leaf, n_node))
    for _ in range(RANDOM_WAVES):      # random waves: every lane on its own, walking or not; and waves of random leaf / node counts
        if rng.random() < 0.5:
            w = rng.integers(0, 1 << 25, 64).astype(np.int32)
            off = rng.random(64) < rng.random()
            w[off] = rng.choice(IDLE, int(off.sum()))
            waves.append(w)
        else:
            n_leaf = int(rng.integers(0, 65)); n_node = int(rng.integers(0, 65 - n_leaf))
            waves.append(_wave(rng, n_leaf, n_node, True))
    node = np.array(waves, np.int32)
    flags = [(d, t, e) for d in (0, 1) for t in THRESHOLDS for e in (0, 1)]
    node = np.repeat(node, len(flags), axis=0)
    f = np.array(flags * len(waves), np.int32)
    return node, f[:, 0].copy(), f[:, 1].copy(), f[:, 2].copy(), [c for c in counts for _ in flags]


@pytest.fixture(scope="module")
def masks(cases):
    import host_kernel
    host_kernel.build()
    return host_kernel.step_masks(*cases[:4])


def _bits(m):
    """uint64[n] -> bool[n, 64], lane l in column l"""
    return ((m[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)


def test_the_cases_cover_the_issue(cases):
    node, draining, leaf_min, exclusive, counts = cases
    have = set(counts)
    for n_leaf in LEAF_COUNTS:
        assert (n_leaf, 0) in have
        if n_leaf <= 63:
            assert (n_leaf, 1) in have
        if n_leaf <= 60:
            assert any(l == n_leaf and n > 1 for l, n in have)
    assert {(int(d), int(t), int(e)) for d, t, e in zip(draining, leaf_min, exclusive)} == {(d, t, e) for d in (0, 1) for t in THRESHOLDS for e in (0, 1)}
    structured = node[:len(counts)]
    for state in IDLE:
        assert (structured == state).any()
    # a non-walking lane of either parity beside leaf lanes and beside node lanes
    mixed = ((structured == LANE_DONE).any(axis=1) & (structured == LANE_REFILL).any(axis=1) & (structured == LANE_RETIRED).any(axis=1))
    assert (mixed & ((structured >= 0) & (structured & 1 == 1)).any(axis=1)).any() and (mixed & ((structured >= 0) & (structured & 1 == 0)).any(axis=1)).any()
    assert len(node) - len(counts) >= 2000 * 8


def test_step_masks_equal_the_per_lane_rule(cases, masks):
    node, draining, leaf_min, exclusive, _ = cases
    walking = node >= 0
    at_leaf = walking & ((node & 1) == 1)
    at_node = walking & ((node & 1) == 0)
    n_leaf, n_node = at_leaf.sum(axis=1), at_node.sum(axis=1)
    drain, excl = draining != 0, exclusive != 0
    do_leaves = (n_leaf > 0) & ((n_leaf >= leaf_min) | (n_node == 0) | drain)
    do_nodes = ~excl | ~do_leaves | drain
    steps = walking & np.where(at_leaf, do_leaves[:, None], do_nodes[:, None])
    as_leaf = steps & at_leaf
    got_step, got_leaf = _bits(masks[0]), _bits(masks[1])
    bad = np.nonzero((got_step != steps).any(axis=1) | (got_leaf != as_leaf).any(axis=1))[0]
    assert bad.size == 0, "first difference: %d leaf and %d node lanes, draining %d, leaf_min %d, exclusive %d: step %#x, leaf %#x" % (
        n_leaf[bad[0]], n_node[bad[0]], draining[bad[0]], leaf_min[bad[0]], exclusive[bad[0]], int(masks[0][bad[0]]), int(masks[1][bad[0]]))
    # the rule's arms were all taken: leaf lanes parked beside stepping node lanes, both kinds together, leaves alone with node lanes sitting out
    parked = (n_leaf > 0) & ~do_leaves
    assert parked.any() and (do_leaves & do_nodes & (n_node > 0)).any() and (do_leaves & ~do_nodes & (n_node > 0)).any() and (~steps.any(axis=1)).any()
