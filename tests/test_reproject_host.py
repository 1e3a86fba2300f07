"""The temporal reprojection without a GPU: the host build of its device functions (tools/host_kernel.cpp hk_reproject = device_reproject.hpp
compiled for the CPU) against the numpy restatement (tests/reproject_checks.py), bit for bit, with guides from the host build of the AOV kernel
(hk_aov); the identity, a synthetic plane moved by whole pixels, the history arithmetic, the parameters and the C layout of the structs."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import CUBE_SETTINGS, ROOT, SCENES, with_settings
import reproject_checks as rc

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


def scene_cases(orc, synth, tmp_path):
    """(name, path, settings13, W, H) for cube, matball, textest and hf_small"""
    cube = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube.rts"), CUBE_SETTINGS)
    textest = os.path.join(SCENES, "textest.rts")
    if not any(l.startswith("*") for l in open(textest)):
        textest = with_settings(textest, str(tmp_path / "textest.rts"), CUBE_SETTINGS)
    out = []
    for name, path, W, H in (("cube", cube, 136, 96), ("matball", os.path.join(synth["dir"], "matball.rts"), 120, 88),
                             ("textest", textest, 136, 96), ("hf_small", os.path.join(synth["dir"], "hf_small.rts"), 160, 96)):
        out.append((name, path, orc.settings13(orc.Scene(path, None).settings(), 1), W, H))
    return out


def random_acc(rng, W, H, gw, gh, lo=-3000, hi=20000):
    acc = np.zeros((W, H, 3), np.int32)
    acc[:gw, :gh] = rng.integers(lo, hi, size=(gw, gh, 3))
    return acc


def both(hk, acc, hist, frames, st_a, st_b, ga, gb, **params):
    """(host build, restatement) on the same inputs, asserted equal; returns the host build's (acc, hist, counts) and the restatement's info"""
    W, H = acc.shape[0], acc.shape[1]
    ca, cb = hk.camera_block(st_a, W, H), hk.camera_block(st_b, W, H)
    got = hk.reproject(acc, hist, frames, st_a, st_b, ga, gb, **params)
    want = rc.reproject(acc, hist, frames, ca, cb, ga, gb, ca["gw"], ca["gh"], **params)
    assert got[2] == want[2], (got[2], want[2])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert sum(got[2][k] for k in rc.CLASSES) == got[2]["pixels"] == ca["gw"] * ca["gh"]
    return got, want[3]


def test_directions_are_the_aov_kernels(hk, orc, synth, tmp_path):
    """d(view, x, y) of the definition is dr_render_aov's `dir` channel, bit for bit"""
    for name, path, st, W, H in scene_cases(orc, synth, tmp_path):
        for view in [st] + list(rc.moves(st).values()):
            cam = hk.camera_block(view, W, H)
            a = hk.Scene(path, "").aov(view, W, H)
            y, x = np.meshgrid(np.arange(cam["gh"]), np.arange(cam["gw"]), indexing="ij")
            assert np.array_equal(rc.directions(cam, x, y).view(np.uint32), a["dir"].view(np.uint32)), name


def test_host_build_equals_the_restatement(hk, orc, synth, tmp_path):
    rng = np.random.default_rng(21)
    seen = {k: 0 for k in rc.CLASSES}
    behind = 0
    for name, path, st, W, H in scene_cases(orc, synth, tmp_path):
        scene = hk.Scene(path, "")
        ga = scene.aov(st, W, H)
        gw, gh = ga["t"].shape[1], ga["t"].shape[0]
        acc = random_acc(rng, W, H, gw, gh)
        hist = np.zeros((W, H), np.int32)
        hist[:gw, :gh] = rng.integers(0, 33, size=(gw, gh))
        for move, st_b in rc.moves(st).items():
            gb = scene.aov(st_b, W, H)
            for h in (None, hist):
                for frames in (1, 5, 40):
                    for mh in (1, 8, 32):
                        (_, hist_to, counts), info = both(hk, acc, h, frames, st, st_b, ga, gb, max_history=mh)
                        assert hist_to.max() <= mh, (name, move)
            for k in rc.CLASSES:
                seen[k] += counts[k]
            if move == "behind":
                behind += info["behind"]
            print("reproject %s %s: %s" % (name, move, counts))
        # the other switches, once per scene
        both(hk, acc, hist, 3, st, st_b, ga, gb, sky=0, material_mask=0xFFFFFFFF)
        both(hk, acc, hist, 3, st, rc.moves(st)["sideways"], ga, scene.aov(rc.moves(st)["sideways"], W, H), normal_cos=0.999, plane_tolerance=0.0005)
    assert all(seen[k] > 0 for k in rc.CLASSES), seen
    assert behind > 0, "no pixel of the `behind` moves lies behind the old camera"


def test_identity(hk, orc, synth, tmp_path):
    rng = np.random.default_rng(3)
    for name, path, st, W, H in scene_cases(orc, synth, tmp_path):
        g = hk.Scene(path, "").aov(st, W, H)
        gw, gh = g["t"].shape[1], g["t"].shape[0]
        acc = random_acc(rng, W, H, gw, gh)
        for params in ({}, {"sky": 0}, {"material_mask": 1}):
            p = dict(rc.DEFAULTS, **params)
            ok = rc.allowed(g["material"], p).T                       # [gw, gh]
            (acc_to, hist_to, counts), info = both(hk, acc, None, 7, st, st, g, g, **params)
            assert counts["valid"] == int(ok.sum()) and counts["masked"] == gw * gh - counts["valid"], (name, params, counts)
            assert np.array_equal(acc_to[:gw, :gh][ok], acc[:gw, :gh][ok]) and (hist_to[:gw, :gh][ok] == 7).all(), (name, params)
            assert not acc_to[:gw, :gh][~ok].any() and not hist_to[:gw, :gh][~ok].any()
            assert not acc_to[gw:].any() and not acc_to[:, gh:].any() and not hist_to[gw:].any() and not hist_to[:, gh:].any()
            y, x = np.meshgrid(np.arange(gh), np.arange(gw), indexing="ij")
            v = info["cls"] == 0
            assert np.array_equal(info["qx"][v], x[v]) and np.array_equal(info["qy"][v], y[v]), name
        # frames beyond max_history: the int64 formula, towards zero
        (acc_to, hist_to, _), _ = both(hk, acc, None, 40, st, st, g, g, max_history=8)
        ok = rc.allowed(g["material"], rc.DEFAULTS).T
        want = np.array([[int(v) * 8 // 40 if v >= 0 else -((-int(v) * 8) // 40) for v in px] for px in acc[:gw, :gh][ok]], np.int32)
        assert np.array_equal(acc_to[:gw, :gh][ok], want) and (hist_to[:gw, :gh][ok] == 8).all(), name
        assert (acc[:gw, :gh][ok] < 0).any()


def plane_view(hk, W, H, shift_pixels=0, depth=5.0):
    """A camera on the z axis looking down -z at the plane z = 0, moved sideways by shift_pixels pixel widths of that plane; its settings13,
    camera block and hand-made guides (one plane facing the camera, one material)"""
    st = np.zeros(13, np.float32)
    st[0:3] = (0, 0, depth)
    st[7], st[8], st[9], st[10], st[11] = 1, 45, 4, 1, 1
    cam = hk.camera_block(st, W, H)
    pw = float(np.linalg.norm(cam["hor"].astype(np.float64))) / cam["den_w"] * depth          # hor spans the image at the focus distance 1
    st[0] = st[3] = np.float32(shift_pixels * pw)
    cam = hk.camera_block(st, W, H)
    y, x = np.meshgrid(np.arange(cam["gh"]), np.arange(cam["gw"]), indexing="ij")
    d = rc.directions(cam, x, y).astype(np.float64)
    g = {"t": (-depth / d[..., 2]).astype(np.float32), "normal": np.zeros((cam["gh"], cam["gw"], 3), np.float32),
         "material": np.zeros((cam["gh"], cam["gw"]), np.int32)}
    g["normal"][..., 2] = 1
    return st, cam, g


def test_synthetic_plane_moves_by_whole_pixels(hk):
    W, H = 128, 96
    rng = np.random.default_rng(6)
    acc = rng.integers(-500, 30000, size=(W, H, 3)).astype(np.int32)
    st_a, cam_a, ga = plane_view(hk, W, H)
    assert (cam_a["gw"], cam_a["gh"]) == (W, H)
    for k in (1, 3, 17):
        st_b, cam_b, gb = plane_view(hk, W, H, shift_pixels=k)
        (acc_to, hist_to, counts), _ = both(hk, acc, None, 4, st_a, st_b, ga, gb)
        assert np.array_equal(acc_to[:W - k], acc[k:]) and (hist_to[:W - k] == 4).all(), k
        assert not acc_to[W - k:].any() and not hist_to[W - k:].any(), k
        assert counts == {"pixels": W * H, "valid": (W - k) * H, "masked": 0, "offscreen": k * H, "rejected": 0}, (k, counts)
        # the plane of the `from` guides raised by 0.5 (tolerance: 0.01 * 5): nothing is the same surface any more
        raised = dict(ga, t=(ga["t"] * np.float32(0.9)))
        (acc_to, hist_to, counts), _ = both(hk, acc, None, 4, st_a, st_b, raised, gb)
        assert counts["valid"] == 0 and counts["rejected"] == (W - k) * H and not acc_to.any() and not hist_to.any(), (k, counts)


def test_history_arithmetic(hk, orc, synth, tmp_path):
    """A -> B -> A with frames in between: the counts add up and stop at max_history; negative sums divide towards zero"""
    rng = np.random.default_rng(9)
    name, path, st_a, W, H = scene_cases(orc, synth, tmp_path)[0]
    scene = hk.Scene(path, "")
    st_b = rc.moves(st_a)["sideways"]
    ga, gb = scene.aov(st_a, W, H), scene.aov(st_b, W, H)
    gw, gh = ga["t"].shape[1], ga["t"].shape[0]
    acc0 = random_acc(rng, W, H, gw, gh)
    (acc1, hist1, c1), _ = both(hk, acc0, None, 3, st_a, st_b, ga, gb, max_history=4)
    assert set(np.unique(hist1)) == {0, 3} and c1["valid"] > 0
    acc1 = acc1 + random_acc(rng, W, H, gw, gh, lo=-200, hi=2000)                  # two more frames in view B
    (acc2, hist2, c2), info = both(hk, acc1, hist1, 2, st_b, st_a, gb, ga, max_history=4)
    assert set(np.unique(hist2)) == {0, 2, 4} and hist2.max() <= 4
    v = (info["cls"] == 0).T                                                    # [gw, gh]
    qx, qy = info["qx"].T[v], info["qy"].T[v]
    cnt = hist1[qx, qy].astype(np.int64) + 2
    src = acc1[qx, qy].astype(np.int64)
    capped = cnt > 4
    assert capped.any() and (~capped).any() and (src[capped] < 0).any()
    assert np.array_equal(acc2[:gw, :gh][v][~capped], src[~capped]) and np.array_equal(hist2[:gw, :gh][v][~capped], cnt[~capped])
    want = np.trunc(src[capped] * 4 / cnt[capped][:, None])                      # exact in float64: |src * 4| < 2^53
    exact = np.sign(src[capped]) * ((np.abs(src[capped]) * 4) // cnt[capped][:, None])
    assert np.array_equal(want.astype(np.int64), exact) and np.array_equal(acc2[:gw, :gh][v][capped], exact)
    assert (hist2[:gw, :gh][v][capped] == 4).all()


def test_bad_parameters(hk, orc, synth, tmp_path):
    name, path, st, W, H = scene_cases(orc, synth, tmp_path)[0]
    g = hk.Scene(path, "").aov(st, W, H)
    acc = np.zeros((W, H, 3), np.int32)
    for bad in ({"max_history": 0}, {"max_history": 65536}, {"normal_cos": 1.5}, {"normal_cos": -1.01}, {"plane_tolerance": -0.1},
                {"normal_cos": float("nan")}):
        with pytest.raises(RuntimeError):
            hk.reproject(acc, None, 1, st, st, g, g, **bad)
        with pytest.raises(ValueError):
            rc.reproject(acc, None, 1, hk.camera_block(st, W, H), hk.camera_block(st, W, H), g, g, g["t"].shape[1], g["t"].shape[0], **bad)
    with pytest.raises(RuntimeError):
        hk.reproject(acc, None, 0, st, st, g, g)
    with pytest.raises(TypeError):
        hk.reproject(acc, None, 1, st, st, g, g, history=3)
    half = st.copy()
    half[11] = 2
    with pytest.raises(RuntimeError, match="divisors"):
        hk.reproject(acc, None, 1, st, half, g, hk.Scene(path, "").aov(half, W, H))
    flat = st.copy()
    flat[7] = 0                                                                 # focus distance 0: the focus plane collapses into the pinhole
    with pytest.raises(RuntimeError, match="degenerate"):
        hk.reproject(acc, None, 1, flat, st, g, g)


def _layout(tmp_path, name, struct, ctype_names):
    hdr = open(os.path.join(ROOT, "include", "dogeray_amd.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n.strip()) for t, names in re.findall(r"(int|float|uint32_t|int64_t)\s+([\w\s,]+);", body) for n in names.split(",")]
    assert [f[1] for f in fields] == [f[0] for f in struct._fields_]
    assert [f[0] for f in fields] == [ctype_names[t] for _, t in struct._fields_]
    src = tmp_path / (name + ".c")
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dogeray_amd.h"\nint main(void) {\n  printf("%%zu", sizeof(%s));\n' % name +
                   "".join('  printf(" %%zu", offsetof(%s, %s));\n' % (name, n) for _, n in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / name)
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got[0] == ctypes.sizeof(struct)
    assert got[1:] == [getattr(struct, n).offset for _, n in fields]


def test_struct_layouts_match_the_header(tmp_path):
    import dogeray_amd as dr
    names = {ctypes.c_int: "int", ctypes.c_float: "float", ctypes.c_uint32: "uint32_t", ctypes.c_int64: "int64_t"}
    _layout(tmp_path, "dr_reproject_params", dr.DrReprojectParams, names)
    _layout(tmp_path, "dr_reproject_result", dr.DrReprojectResult, names)
    assert [f[0] for f in dr.DrReprojectParams._fields_] == list(rc.DEFAULTS)
    # the library's defaults are the restatement's and the host build's (dr_reproject_defaults needs no GPU)
    p = dr.reproject_params()
    got = {k: getattr(p, k) for k in rc.DEFAULTS}
    assert got["max_history"] == 32 and got["material_mask"] == 0xFFFFFFC3 and got["sky"] == 1
    assert got["normal_cos"] == np.float32(0.9) and got["plane_tolerance"] == np.float32(0.01)
    assert {k: (np.float32(v) if isinstance(v, float) else v) for k, v in rc.DEFAULTS.items()} == got
    import host_kernel
    assert host_kernel.REPROJECT_DEFAULTS == rc.DEFAULTS
    with pytest.raises(TypeError):
        dr.reproject_params(history=3)
