"""launch_plan.hpp plan_trace (which kernel dr_trace_rays runs, with what grid) through the host build: a table of (n, traversal, has-wide-tree,
option trace_kernel) against the kernel, the traversal really walked and the workgroups the plan picks.  No GPU."""
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

THREADED, ORDERED, WIDE = 0, 1, 2
PLAIN, PERSISTENT = 0, 1
CUS = 256


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


def test_the_threshold_is_the_measured_one(hk):
    """profiles/trace_rays_rate.txt, part c: the constant is the one the measurement's file names"""
    text = open(os.path.join(ROOT, "profiles", "trace_rays_rate.txt")).read()
    assert "TRACE_PERSISTENT_MIN_RAYS = %d" % hk.trace_persistent_min_rays() in text


def test_plan_table(hk):
    m = hk.trace_persistent_min_rays()
    assert 10 ** 7 < m < 10 ** 9
    full = CUS * 6
    table = [
        # n, traversal, has wide, force -> kernel, traversal walked, blocks
        (1, WIDE, True, 0, PLAIN, WIDE, 1),
        (256, WIDE, True, 0, PLAIN, WIDE, 1),
        (257, WIDE, True, 0, PLAIN, WIDE, 2),
        (m - 1, WIDE, True, 0, PLAIN, WIDE, (m - 1 + 255) // 256),
        (m, WIDE, True, 0, PERSISTENT, WIDE, min(full, (m + 511) // 512)),
        (10 ** 7, WIDE, True, 0, PLAIN, WIDE, (10 ** 7 + 255) // 256),
        (10 ** 9, WIDE, True, 0, PERSISTENT, WIDE, full),
        (2 ** 31 - 1, WIDE, True, 0, PERSISTENT, WIDE, full),
        (2 ** 31 - 1, THREADED, True, 0, PLAIN, THREADED, 2 ** 23),
        # the persistent kernel exists for the wide walk over a wide tree only
        (10 ** 7, WIDE, False, 0, PLAIN, THREADED, (10 ** 7 + 255) // 256),
        (10 ** 7, THREADED, True, 0, PLAIN, THREADED, (10 ** 7 + 255) // 256),
        (10 ** 7, ORDERED, True, 0, PLAIN, ORDERED, (10 ** 7 + 255) // 256),
        (10 ** 7, ORDERED, False, 0, PLAIN, ORDERED, (10 ** 7 + 255) // 256),
        # option trace_kernel: 1 one ray per lane, 2 the persistent kernel where it exists
        (10 ** 7, WIDE, True, 1, PLAIN, WIDE, (10 ** 7 + 255) // 256),
        (1, WIDE, True, 2, PERSISTENT, WIDE, 1),
        (512, WIDE, True, 2, PERSISTENT, WIDE, 1),
        (513, WIDE, True, 2, PERSISTENT, WIDE, 2),
        (1000, WIDE, True, 2, PERSISTENT, WIDE, 2),
        (1000, WIDE, False, 2, PLAIN, THREADED, 4),
        (1000, THREADED, True, 2, PLAIN, THREADED, 4),
        (1000, ORDERED, True, 2, PLAIN, ORDERED, 4),
    ]
    for n, traversal, has_wide, force, kernel, walked, blocks in table:
        assert hk.trace_plan(n, traversal, has_wide, CUS, force) == (kernel, walked, blocks), (n, traversal, has_wide, force)


def test_the_persistent_grid_follows_the_device(hk):
    for cus in (1, 64, 256, 304):
        assert hk.trace_plan(10 ** 9, WIDE, True, cus, 0) == (PERSISTENT, WIDE, cus * 6)
