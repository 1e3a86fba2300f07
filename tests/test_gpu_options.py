"""dr_context_set_option / dr_context_get_option / DOGERAY_OPTIONS on a fresh context: defaults, accepted and refused values, read-only names.

The expected values are the defaults documented in include/dogeray_amd.h and the ranges the setter has always enforced, written out here by hand:
the test pins the behaviour of the option code, it does not read it.
"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

# name: (documented default, [(value set, value read back)], [values refused]); no refused value = the option stores value != 0
SETTABLE = {
    "kernel": (1, [(0, 0), (1, 1)], [-1, 2]),
    "batch_frames": (32, [(1, 1), (256, 256)], [0, 257]),
    "feedback": (1, [(0, 0), (5, 1), (-3, 1)], []),
    "feedback_every": (8, [(1, 1), (1000, 1000)], [0, -1]),
    "order_follows_camera": (1, [(0, 0), (5, 1), (-3, 1)], []),
    "occupancy": (6, [(4, 4), (5, 5)], [3, 7]),
    "schedule": (0, [(1, 1), (2, 2)], [-1, 3]),
    "xcd_regions": (1, [(0, 0), (5, 1), (-3, 1)], []),
    "heavy_factor": (1, [(-1, -1), (0, 0), (1000, 1000)], [-2, 1001]),
    "coop_steps": (2, [(0, 0), (77, 77)], [-1]),
    "coop_rounds": (2, [(1, 1), (16, 16)], [0, 17]),
    "coop_tiles_per_wave": (32, [(0, 0), (500, 500)], [-1]),
    "short_one_queue": (1, [(0, 0), (5, 1), (-3, 1)], []),
    "split_parts": (4, [(1, 1), (2, 2), (8, 8)], [0, 3, 16]),
    "split_steps": (400, [(100, 96), (16, 16), (4080, 4080), (4079, 4064)], [15, 4081]),
    "split_waves": (12, [(1, 1), (1000, 1000)], [0, 1001]),
    "coop_lanes": (8, [(1, 1), (64, 64)], [0, 65]),
    "pipe_streams": (2, [(4, 4), (3, 3)], [1, 5]),
    "pipe_group": (8, [(1, 1), (16, 16)], [0, 17]),
    "pipe_lean": (0, [(5, 1), (0, 0), (-3, 1)], []),
    "reserve_cus": (0, [(64, 64), (1, 1)], [-1, 65]),
    "wave_log": (0, [(1, 1), (0, 0)], [-1, 2]),
    "wide_tree": (2, [(0, 0), (1, 1)], [-1, 3]),
    "denoise_tiles": (1, [(0, 0)], [-1, 2]),
    "camera_cert": (1, [(0, 0)], [-1, 2]),
    "cert_factor": (40, [(1, 1), (10000, 10000)], [0, 10001]),
    "moments": (0, [(1, 1)], [-1, 2]),
    "denoise_variance": (0, [(1, 1)], [-1, 2]),
}
# name: value without a scene
READ_ONLY = {"tree_depth": 0, "wide_own_bounds": 0, "wide_depth": 0, "wide_nodes": 0, "cert_flagged_permille": -1, "upscale_aov_passes": 0,
             "reproject_aov_passes": 0, "traversal": 0}      # (the wide walk has no structure to walk yet: launches would walk threaded, 0)


def test_every_option_default_range_and_read_only_name():
    import dogeray_amd as dr
    assert len(SETTABLE) == 28 and len(READ_ONLY) == 8
    ctx = dr.Context(0)
    try:
        for name, (default, _, _) in SETTABLE.items():
            assert ctx.get_option(name) == default, name
        for name, (default, accepted, refused) in SETTABLE.items():
            assert any(back != default for _, back in accepted), name
            for v, back in accepted:
                ctx.set_option(name, v)
                assert ctx.get_option(name) == back, (name, v)
                for bad in refused:
                    with pytest.raises(dr.DogerayError) as e:
                        ctx.set_option(name, bad)
                    assert e.value.code == dr.ERR_INVALID, (name, bad)
                    assert "value not supported for option '%s'" % name in str(e.value), (name, bad)
                    assert ctx.get_option(name) == back, (name, bad)
            ctx.set_option(name, default)
            assert ctx.get_option(name) == default, name
        for name, want in READ_ONLY.items():
            with pytest.raises(dr.DogerayError) as e:
                ctx.set_option(name, 1)
            assert e.value.code == dr.ERR_INVALID and "unknown option '%s'" % name in str(e.value), name
            assert ctx.get_option(name) == want, name
        with pytest.raises(dr.DogerayError) as e:
            ctx.get_option("no_such_option")
        assert e.value.code == dr.ERR_INVALID and str(e.value).endswith("unknown option no_such_option")
        # nothing above moved another option
        for name, (default, _, _) in SETTABLE.items():
            assert ctx.get_option(name) == default, name
    finally:
        ctx.close()


CHILD = """
import sys
sys.path.insert(0, %r)
import dogeray_amd as dr
try:
    c = dr.Context(0)
except dr.DogerayError as e:
    print("code", e.code, e)
else:
    print("created", c.get_option("occupancy"), c.get_option("split_steps"), c.get_option("pipe_lean"))
    c.close()
"""


@pytest.mark.parametrize("options,want", [
    ("occupancy=7", "code -1 "),                                   # a refused value: dr_context_create fails with DR_ERR_INVALID
    ("occupancy=4,split_steps=100,pipe_lean=5", "created 4 96 1"),
])
def test_dogeray_options_environment(options, want):
    env = dict(os.environ, DOGERAY_OPTIONS=options)
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith(want), (r.stdout, r.stderr)
    if want.startswith("code"):
        assert "option '" in r.stdout, r.stdout
