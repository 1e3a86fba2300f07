"""launch_plan.hpp plan_trace, plan_radiance and plan_allhits share one planner (plan_ray_list).  Through the host build's exports each must return what
its own formula returned before they were folded; the formulas are written out here in plain Python, with each query's constants.  No GPU."""
import itertools
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

THREADED, ORDERED, WIDE = 0, 1, 2
PLAIN, PERSISTENT = 0, 1
# waves per SIMD, rays per chunk, the measured cross-over (launch_plan.hpp TRACE_*, RADIANCE_*, ALLHITS_*)
TRACE = (6, 128, 1 << 25)
RADIANCE = (5, 64, 1 << 22)
ALLHITS = (5, 128, 1 << 23)


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


def ray_list(n, can_persist, force, consts, num_cus):
    """(kernel, workgroups) as the three planners each spelled it"""
    occ, chunk, min_rays = consts
    persistent = can_persist and (force == 2 or (force != 1 and n >= min_rays))
    if persistent:      # no more waves than chunks
        return PERSISTENT, min(num_cus * occ, (n + 4 * chunk - 1) // (4 * chunk))
    return PLAIN, (n + 255) // 256


def walked(traversal, has_wide):
    return THREADED if traversal == WIDE and not has_wide else traversal


def counts(consts):
    occ, chunk, min_rays = consts
    return (1, 255, 256, 257, chunk * 4 - 1, chunk * 4, chunk * 4 + 1, min_rays - 1, min_rays)


GRID = list(itertools.product((1, 256, 320), (0, 1, 2), (False, True)))


def test_the_constants_are_the_headers(hk):
    assert (hk.trace_persistent_min_rays(), hk.radiance_persistent_min_rays(), hk.allhits_persistent_min_rays()) == (TRACE[2], RADIANCE[2], ALLHITS[2])
    assert (hk.radiance_occ(), hk.radiance_chunk(), hk.allhits_chunk()) == (RADIANCE[0], RADIANCE[1], ALLHITS[1])


@pytest.mark.parametrize("name, consts", [("trace_plan", TRACE), ("radiance_plan", RADIANCE)])
def test_trace_and_radiance_plans(hk, name, consts):
    plan = getattr(hk, name)
    for n in counts(consts):
        for (cus, force, has_wide), traversal in itertools.product(GRID, (THREADED, ORDERED, WIDE)):
            walk = walked(traversal, has_wide)
            kernel, blocks = ray_list(n, walk == WIDE, force, consts, cus)
            assert plan(n, traversal, has_wide, cus, force) == (kernel, walk, blocks), (n, traversal, has_wide, cus, force)


def test_allhits_plan(hk):
    for n in counts(ALLHITS):
        for cus, force, has_wide in GRID:
            kernel, blocks = ray_list(n, has_wide, force, ALLHITS, cus)
            assert hk.allhits_plan(n, has_wide, cus, force) == (kernel, int(has_wide), blocks), (n, has_wide, cus, force)
