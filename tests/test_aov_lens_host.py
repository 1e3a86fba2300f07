"""Lens-averaged AOVs without a GPU: the host build of the per-pixel body (tools/host_kernel.cpp hk_aov_lens = device_aov_lens.hpp aov_lens_pixel
compiled for the CPU) against the numpy fold of the host build's own camera rays and ray-surface answers (tests/aov_lens_checks.py), bit for
bit; what a single sample and a material imply; windows, the guide form, the refusals and the C layout of dr_aov_lens_buffers."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import aov_lens_checks as lc

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


def _settings(orc, path):
    o = orc.Scene(path, None)
    return np.array(orc.settings13(o.settings(), 1), dtype=np.float32)


@pytest.mark.parametrize("aperture,spp,nframes", [(0.5, 2, 3), (0.0, 2, 3), (0.5, 1, 1)])
def test_host_build_equals_the_fold(hk, orc, synth, tmp_path, aperture, spp, nframes):
    for name, path in lc.scene_paths(synth, tmp_path):
        st = lc.lens_settings(_settings(orc, path), aperture, spp)
        sc = hk.Scene(path, "")
        gw, gh = lc.W // 8 * 8, lc.H // 8 * 8
        what = "%s aperture %g spp %d nframes %d" % (name, aperture, spp, nframes)
        for as_guides in (False, True):
            want = lc.fold(hk.kat_camera, sc.trace, st, lc.W, lc.H, (0, 0, gw, gh), lc.SEED, lc.STRIDE, nframes, as_guides)
            for traversal in ((2, 0, 1) if not as_guides else (2,)):
                got = sc.aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, nframes, as_guides=as_guides, traversal=traversal)
                lc.assert_same(got, want, "%s traversal %d guides %d" % (what, traversal, as_guides))
                lc.check_properties(got, what)
        plain = sc.aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, nframes)
        assert (plain["coverage"] > 0).any() and (plain["material"] != -1).any(), what
        if aperture > 0 and nframes * spp > 1:
            part = (plain["coverage"] > 0) & (plain["coverage"] < 1)
            assert part.any(), "%s: no pixel is partly covered" % what


def test_one_sample_is_the_single_ray(hk, orc, synth, tmp_path):
    """N = 1: every channel is the one camera ray's own answer"""
    for name, path in lc.scene_paths(synth, tmp_path):
        st = lc.lens_settings(_settings(orc, path), 0.5, 1)
        sc = hk.Scene(path, "")
        gw, gh = lc.W // 8 * 8, lc.H // 8 * 8
        a = sc.aov_lens(st, lc.W, lc.H, 99, 7, 1)
        yy, xx = np.mgrid[0:gh, 0:gw]
        x, y = xx.ravel().astype(np.int32), yy.ravel().astype(np.int32)
        cam = hk.kat_camera(st, lc.W, lc.H, 99, 8 * (lc.W // 8), x, y, np.zeros(x.size, np.int32))
        r = sc.trace(np.ascontiguousarray(cam[0][0]), np.ascontiguousarray(cam[1][0]), channels=lc.SURFACE)
        hit = (r["t"] > 0).reshape(gh, gw)
        assert hit.any() and (~hit).any(), name
        assert np.array_equal(a["coverage"], hit.astype(np.float32)), name
        assert np.array_equal(a["material"], r["material"].reshape(gh, gw)), name
        t = r["t"].reshape(gh, gw)
        assert np.array_equal(lc.bits(a["depth"][hit]), lc.bits((t[hit] * np.float32(st[7])).astype(np.float32))), name
        assert np.array_equal(lc.bits(a["distance"]), lc.bits(r["distance"].reshape(gh, gw))), name
        zero = np.float32(0)                    # (the sums start from 0: a component of -0 comes back as 0 + -0 = +0)
        assert np.array_equal(lc.bits(a["normal"]), lc.bits(zero + r["normal"].reshape(gh, gw, 3))), name
        assert np.array_equal(lc.bits(a["albedo"]), lc.bits(zero + r["albedo"].reshape(gh, gw, 3))), name
        assert np.isposinf(a["depth"][~hit]).all(), name


def test_window_is_the_crop_and_the_refusals(hk, orc, synth, tmp_path):
    name, path = lc.scene_paths(synth, tmp_path)[1]
    st = lc.lens_settings(_settings(orc, path), 0.5, 2)
    sc = hk.Scene(path, "")
    full = sc.aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, 3)
    x0, y0, w, h = lc.WINDOW
    win = sc.aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, 3, window=lc.WINDOW)
    lc.assert_same(win, {k: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w]) for k, a in full.items()}, "window")
    for nframes in (0, 129, -1):             # N = 0, 258
        with pytest.raises(RuntimeError, match="samples"):
            sc.aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, nframes)
    with pytest.raises(RuntimeError, match="window"):
        sc.aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, 1, window=(70, 0, 8, 8))
    sc.aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, 128, window=(8, 8, 2, 2))      # N = 256 is accepted


def test_lens_buffers_layout_and_the_header(tmp_path):
    import dogeray_amd as dr
    hdr = open(os.path.join(ROOT, "include", "dogeray_amd.h")).read()
    body = re.search(r"typedef struct dr_aov_lens_buffers \{(.*?)\} dr_aov_lens_buffers;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"\*\s*(\w+)\s*;", body)
    assert names == [f[0] for f in dr.DrAovLensBuffers._fields_] == list(lc.CHANNELS) == list(dr.AOV_LENS_CHANNELS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dogeray_amd.h"\nint main(void) {\n  printf("%zu %llu", sizeof(dr_aov_lens_buffers), '
                   "(unsigned long long)DR_GUIDE_SEED);\n" +
                   "".join('  printf(" %%zu", offsetof(dr_aov_lens_buffers, %s));\n' % n for n in names) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got[0] == ctypes.sizeof(dr.DrAovLensBuffers) and got[1] == dr.GUIDE_SEED
    assert got[2:] == [getattr(dr.DrAovLensBuffers, n).offset for n in names]
    assert "dr_render_aov_lens" in dr.API_SYMBOLS and '"guide_frames"' in hdr and "DESIGN.md 4.22" in hdr
