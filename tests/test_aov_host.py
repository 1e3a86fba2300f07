"""First-hit AOV buffers without a GPU: the host build of the device function (tools/host_kernel.cpp hk_aov = device_aov.hpp aov_first_hit
compiled for the CPU) against the oracle and numpy restatements, the C layout of dr_aov_buffers, the PFM helpers."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import aov_checks

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


@pytest.mark.parametrize("traversal", [2, 0, 1])
def test_host_aov_matches_the_oracle(hk, orc, synth, tmp_path, traversal):
    for name, path, tex, W, H in aov_checks.scene_cases(synth, tmp_path):
        o = orc.Scene(path, tex or None)
        o.build_bvh()
        st = orc.settings13(o.settings(), 1)
        a = hk.Scene(path, tex).aov(st, W, H, traversal=traversal)
        assert a["t"].shape == (H // 8 * 8, W // 8 * 8)
        hits = aov_checks.check_against_oracle(a, o, st, W, H, (0, 0, W // 8 * 8, H // 8 * 8), "%s traversal %d" % (name, traversal))
        assert hits > 0


def test_host_aov_window_and_divisor(hk, orc, synth):
    """A window is the crop of the full grid; with divisor 2 the grid is the half-size one dr_render_frame renders."""
    path = os.path.join(synth["dir"], "city_small.rts")
    o = orc.Scene(path)
    o.build_bvh()
    st = orc.settings13(o.settings(), 1)
    sc = hk.Scene(path, "")
    full = sc.aov(st, 160, 96)
    win = sc.aov(st, 160, 96, window=(17, 9, 33, 21))
    for k in aov_checks.CHANNELS:
        assert np.array_equal(win[k].view(np.uint32) if win[k].dtype == np.float32 else win[k],
                              full[k][9:30, 17:50].view(np.uint32) if full[k].dtype == np.float32 else full[k][9:30, 17:50]), k
    st2 = orc.settings13(o.settings(), 2)
    half = sc.aov(st2, 160, 96)
    assert half["t"].shape == (48, 80)
    aov_checks.check_against_oracle(half, o, st2, 160, 96, (0, 0, 80, 48), "divisor 2")
    with pytest.raises(RuntimeError):
        sc.aov(st, 160, 96, window=(150, 0, 16, 8))


def test_aov_buffers_layout_matches_the_header(tmp_path):
    import dogeray_amd as dr
    hdr = open(os.path.join(ROOT, "include", "dogeray_amd.h")).read()
    body = re.search(r"typedef struct dr_aov_buffers \{(.*?)\} dr_aov_buffers;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*\s*(\w+)\s*;", body)
    assert names == [f[0] for f in dr.DrAovBuffers._fields_] == list(aov_checks.CHANNELS) == list(dr.AOV_CHANNELS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dogeray_amd.h"\nint main(void) {\n  printf("%zu", sizeof(dr_aov_buffers));\n' +
                   "".join('  printf(" %%zu", offsetof(dr_aov_buffers, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got[0] == ctypes.sizeof(dr.DrAovBuffers)
    assert got[1:] == [getattr(dr.DrAovBuffers, n).offset for n in names]


def test_pfm_round_trip(tmp_path):
    import dogeray_amd as dr
    rng = np.random.default_rng(3)
    for shape in ((5, 7), (4, 9, 3), (1, 1)):
        a = rng.normal(size=shape).astype(np.float32)
        a.flat[0] = np.inf
        p = str(tmp_path / "a.pfm")
        dr.write_pfm(p, a)
        b = dr.read_pfm(p)
        assert b.dtype == np.float32 and b.shape == a.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        head = open(p, "rb").read(2)
        assert head == (b"PF" if a.ndim == 3 else b"Pf")
    # the file stores the bottom row first
    a = np.arange(6, dtype=np.float32).reshape(2, 3)
    dr.write_pfm(p, a)
    raw = open(p, "rb").read()
    assert np.array_equal(np.frombuffer(raw[-24:], "<f4"), np.array([3, 4, 5, 0, 1, 2], np.float32))


def test_pixel_grid_is_the_render_grid():
    import dogeray_amd as dr
    st = np.zeros(13, np.float32)
    for div, W, H, want in ((1, 256, 256, (256, 256)), (2, 37, 23, (16, 8)), (1, 7, 200, (0, 200)), (8, 1920, 1080, (240, 128))):
        st[11] = div
        assert dr.pixel_grid(st, W, H) == want
    st[11] = 0
    assert dr.pixel_grid(st, 64, 64) == (0, 0)
