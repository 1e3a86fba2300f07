"""The a-trous denoiser without a GPU: the host build of its device functions (tools/host_kernel.cpp hk_denoise = device_denoise.hpp compiled for
the CPU) against the numpy restatement (tests/denoise_checks.py), bit for bit, with guides from the host build of the AOV kernel (hk_aov);
the edge stops' invariances, the integer present at 0 iterations, and the C layout of dr_denoise_params."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import CUBE_SETTINGS, ROOT, SCENES, with_settings
import denoise_checks as dc

sys.path.insert(0, os.path.join(ROOT, "tools"))

SWITCHES = ({}, {"demodulate": 0}, {"material_stop": 0}, {"sigma_luminance": 0.0, "sigma_depth": 0.0, "normal_power_log2": 0})


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


def guide_cases(hk, orc, synth, tmp_path, div=1):
    """(name, settings13, W, H, AOVs of the grid) for cube, matball, textest and hf_small"""
    cube = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube.rts"), CUBE_SETTINGS)
    textest = os.path.join(SCENES, "textest.rts")
    if not any(l.startswith("*") for l in open(textest)):
        textest = with_settings(textest, str(tmp_path / "textest.rts"), CUBE_SETTINGS)
    out = []
    for name, path, tex, W, H in (("cube", cube, "", 136, 96), ("matball", os.path.join(synth["dir"], "matball.rts"), "", 120, 88),
                                  ("textest", textest, "", 136, 96), ("hf_small", os.path.join(synth["dir"], "hf_small.rts"), "", 160, 96)):
        o = orc.Scene(path, tex or None)
        st = orc.settings13(o.settings(), div)
        out.append((name, st, W, H, hk.Scene(path, tex).aov(st, W, H)))
    return out


def random_acc(rng, W, H, gw, gh, hi=20000):
    acc = np.zeros((W, H, 3), np.int32)
    acc[:gw, :gh] = rng.integers(0, hi, size=(gw, gh, 3))
    return acc


def both(hk, acc, st, div, a, **params):
    g = (a["normal"], a["albedo"], a["depth"], a["material"])
    return hk.denoise(acc, st, div, *g, **params), dc.denoise(acc, st, div, *g, **params)


def test_host_build_equals_the_restatement(hk, orc, synth, tmp_path):
    rng = np.random.default_rng(11)
    for name, st, W, H, a in guide_cases(hk, orc, synth, tmp_path):
        gw, gh = dc.grid(st, W, H)
        assert (a["material"] == -1).any() and (a["material"] >= 0).any(), name
        acc = random_acc(rng, W, H, gw, gh)
        for it in range(6):
            for sw in SWITCHES:
                (f1, r1), (f2, r2) = both(hk, acc, st, 9, a, iterations=it, **sw)
                what = "%s iterations %d %s" % (name, it, sw)
                assert dc.same_bits(f1, f2), "%s: f32 differs at %d values" % (what, int((dc.bits(f1) != dc.bits(f2)).sum()))
                assert np.array_equal(r1, r2), what
                assert np.isfinite(f1).all() and not f1[gh:].any() and not f1[:, gw:].any(), what


def test_preview_grid_and_ten_iterations(hk, orc, synth, tmp_path):
    """div 2: a quarter of the accumulator is the grid; 10 iterations reach taps 1024 pixels away (all outside)"""
    rng = np.random.default_rng(5)
    for name, st, W, H, a in guide_cases(hk, orc, synth, tmp_path, div=2)[:2]:
        gw, gh = dc.grid(st, W, H)
        assert a["depth"].shape == (gh, gw) and gw < W
        acc = random_acc(rng, W, H, gw, gh)
        for it in (3, 10):
            (f1, r1), (f2, r2) = both(hk, acc, st, 3, a, iterations=it)
            assert dc.same_bits(f1, f2) and np.array_equal(r1, r2), (name, it)


def test_zero_iterations_is_the_integer_present(hk, orc, synth, tmp_path):
    rng = np.random.default_rng(2)
    name, st, W, H, a = guide_cases(hk, orc, synth, tmp_path)[0]
    gw, gh = dc.grid(st, W, H)
    acc = random_acc(rng, W, H, gw, gh, hi=1 << 24)
    acc[:gw, :gh][rng.random((gw, gh, 3)) < 0.05] *= -1
    for div in (1, 2, 3, 7, 255, 256, 257, 1000, 65535):
        (f1, r1), (f2, r2) = both(hk, acc, st, div, a, iterations=0)
        present = np.clip(np.trunc(acc.astype(np.int64) / div), 0, 255).astype(np.uint8).transpose(1, 0, 2)
        assert np.array_equal(r1, present) and np.array_equal(r2, present), div
        assert dc.same_bits(f1[:gh, :gw], (acc[:gw, :gh].astype(np.float32) / np.float32(div)).transpose(1, 0, 2)), div


def test_edge_stops_are_exact(hk, orc, synth, tmp_path):
    """With material_stop, new colours on the pixels of one material leave every other material's output bits as they were; hit pixels and
    misses never see each other's colour, with or without material_stop."""
    rng = np.random.default_rng(8)
    for name, st, W, H, a in guide_cases(hk, orc, synth, tmp_path):
        gw, gh = dc.grid(st, W, H)
        m = a["material"]
        acc = random_acc(rng, W, H, gw, gh)
        mats = [v for v in np.unique(m) if v >= 0]
        base, _ = hk.denoise(acc, st, 4, a["normal"], a["albedo"], a["depth"], m)
        if len(mats) > 1:
            b = mats[-1]
            acc2 = acc.copy()
            sel = (m == b).T
            acc2[:gw, :gh][sel] = rng.integers(0, 20000, size=(int(sel.sum()), 3))
            f2, _ = hk.denoise(acc2, st, 4, a["normal"], a["albedo"], a["depth"], m)
            keep = m != b
            assert dc.same_bits(f2[:gh, :gw][keep], base[:gh, :gw][keep]), name
            assert not np.array_equal(f2[:gh, :gw][~keep], base[:gh, :gw][~keep]), name
        for mstop in (1, 0):
            base, _ = hk.denoise(acc, st, 4, a["normal"], a["albedo"], a["depth"], m, material_stop=mstop)
            for changed in (m == -1, m != -1):
                acc2 = acc.copy()
                acc2[:gw, :gh][changed.T] = rng.integers(0, 20000, size=(int(changed.sum()), 3))
                f2, _ = hk.denoise(acc2, st, 4, a["normal"], a["albedo"], a["depth"], m, material_stop=mstop)
                assert dc.same_bits(f2[:gh, :gw][~changed], base[:gh, :gw][~changed]), (name, mstop)


def test_flat_guides_remove_noise(hk):
    """Flat guides (one plane facing the camera, one material): white noise around a grey level loses at least 4x of its variance"""
    W, H = 128, 96
    st = np.zeros(13, np.float32)
    st[11] = 1
    rng = np.random.default_rng(4)
    normal = np.zeros((H, W, 3), np.float32)
    normal[..., 2] = 1
    albedo = np.full((H, W, 3), 0.5, np.float32)
    depth = np.full((H, W), 5.0, np.float32)
    mat = np.zeros((H, W), np.int32)
    acc = rng.normal(100 * 8, 30 * 8, size=(W, H, 3)).astype(np.int32)
    f0, _ = hk.denoise(acc, st, 8, normal, albedo, depth, mat, iterations=0)
    f5, r5 = hk.denoise(acc, st, 8, normal, albedo, depth, mat, iterations=5)
    f5n, r5n = dc.denoise(acc, st, 8, normal, albedo, depth, mat, iterations=5)
    assert dc.same_bits(f5, f5n) and np.array_equal(r5, r5n)
    v0, v5 = float(f0.var()), float(f5.var())
    assert v5 * 4 <= v0, (v0, v5)
    assert abs(float(f5.mean()) - float(f0.mean())) < 1.0


def test_bad_parameters(hk, orc, synth, tmp_path):
    name, st, W, H, a = guide_cases(hk, orc, synth, tmp_path)[0]
    acc = np.zeros((W, H, 3), np.int32)
    g = (a["normal"], a["albedo"], a["depth"], a["material"])
    for bad in ({"iterations": 11}, {"iterations": -1}, {"sigma_luminance": -1.0}, {"sigma_depth": -0.5}, {"normal_power_log2": 17}):
        with pytest.raises(RuntimeError):
            hk.denoise(acc, st, 1, *g, **bad)
    with pytest.raises(RuntimeError):
        hk.denoise(acc, st, 0, *g)


def test_denoise_params_layout_matches_the_header(tmp_path):
    import dogeray_amd as dr
    hdr = open(os.path.join(ROOT, "include", "dogeray_amd.h")).read()
    body = re.search(r"typedef struct dr_denoise_params \{(.*?)\} dr_denoise_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int|float)\s+(\w+)\s*;", body)
    assert [f[1] for f in fields] == [f[0] for f in dr.DrDenoiseParams._fields_] == list(dc.DEFAULTS)
    assert [f[0] for f in fields] == ["float" if t is ctypes.c_float else "int" for _, t in dr.DrDenoiseParams._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dogeray_amd.h"\nint main(void) {\n  printf("%zu", sizeof(dr_denoise_params));\n' +
                   "".join('  printf(" %%zu", offsetof(dr_denoise_params, %s));\n' % n for _, n in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got[0] == ctypes.sizeof(dr.DrDenoiseParams)
    assert got[1:] == [getattr(dr.DrDenoiseParams, n).offset for _, n in fields]
    # the library's defaults are the restatement's (dr_denoise_defaults needs no GPU)
    p = dr.denoise_params()
    assert {k: getattr(p, k) for k in dc.DEFAULTS} == dc.DEFAULTS
