"""The second-moment plane without a GPU: the host build of its device functions (tools/host_kernel.cpp hk_moments_add / hk_error /
hk_reproject / hk_denoise = device_moments.hpp compiled for the CPU) against the numpy restatement (tests/moments_checks.py), bit for
bit, on frames rendered by the host build of the render kernel and on synthetic frames that reach the cap and the saturation; the carry across
a reprojection, the denoiser's temporal variance, the C layout of dr_error_result and the surface (symbols, options, the CLI's help)."""
import ctypes
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import CUBE_SETTINGS, ROOT, SCENES, with_settings
import denoise_checks as dc
import moments_checks as mc
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
    """(name, path, settings13, background, W, H) for cube, matball and textest"""
    cube = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube.rts"), CUBE_SETTINGS)
    textest = os.path.join(SCENES, "textest.rts")
    if not any(l.startswith("*") for l in open(textest)):
        textest = with_settings(textest, str(tmp_path / "textest.rts"), CUBE_SETTINGS)
    out = []
    for name, path, W, H in (("cube", cube, 136, 96), ("matball", os.path.join(synth["dir"], "matball.rts"), 120, 88), ("textest", textest, 136, 96)):
        s = orc.Scene(path, None).settings()
        out.append((name, path, orc.settings13(s, 1), s.background, W, H))
    return out


def accumulate(hk, scene, st, bg, W, H, nframes, seed=100, checkpoints=()):
    """nframes frames of the host render kernel folded by hk_moments_add and by the restatement, asserted equal after every frame; returns
    (acc, m2, the frames, {n: (acc, m2) copies at the checkpoints})"""
    acc, m2 = np.zeros((W, H, 3), np.int32), np.zeros((W, H), np.uint64)
    want_acc, want_m2 = acc.copy(), m2.copy()
    frames, kept = [], {}
    for k in range(nframes):
        f, _ = scene.render(st, W, H, bg, seed + 7919 * k, nthreads=4, count=False)
        frames.append(f)
        hk.moments_add(acc, m2, f)
        want_acc, want_m2 = mc.add(want_acc, want_m2, f)
        assert np.array_equal(acc, want_acc) and np.array_equal(m2, want_m2), k
        if k + 1 in checkpoints:
            kept[k + 1] = (acc.copy(), m2.copy())
    return acc, m2, frames, kept


def test_add_equals_the_restatement_on_rendered_frames(hk, orc, synth, tmp_path):
    for name, path, st, bg, W, H in scene_cases(orc, synth, tmp_path):
        acc, m2, frames, _ = accumulate(hk, hk.Scene(path, ""), st, bg, W, H, 3)
        assert m2.any() and acc.any(), name
        # S1 from the sums is the sum of y exactly when nothing was capped
        assert not any(mc.capped(f).any() for f in frames), name
        assert np.array_equal(mc.luma(acc), sum(mc.luma(f) for f in frames)), name
        assert np.array_equal(m2, sum((mc.luma(f) ** 2).astype(np.uint64) for f in frames)), name


def test_add_cap_negative_values_and_saturation(hk):
    rng = np.random.default_rng(4)
    W, H = 37, 11                                       # W * H % 4 = 3
    frame = rng.integers(-70000, 70000, size=(W, H, 3)).astype(np.int32)
    frame[0, 0] = (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)           # y far above the cap
    frame[0, 1] = (-2 ** 31, -2 ** 31, -2 ** 31)                   # ... and far below
    frame[0, 2] = (0, 366716, 0)                                   # y = 2^26 + 164: just capped
    frame[0, 3] = (0, 366715, 0)                                   # y = 2^26 - 19: just not
    frame[0, 4] = (-300, -5, -7)
    acc = rng.integers(-10 ** 6, 10 ** 6, size=(W, H, 3)).astype(np.int32)
    m2 = rng.integers(0, 2 ** 62, size=(W, H), dtype=np.uint64)
    m2[1, 0] = 2 ** 64 - 1                                         # stays saturated
    m2[1, 1] = 2 ** 64 - 5                                         # saturates unless the frame is black there
    frame[1, 1] = (1, 1, 1)
    m2[1, 2] = 2 ** 64 - 1 - 256 ** 2                              # reaches 2^64 - 1 exactly, without wrapping
    frame[1, 2] = (1, 1, 1)
    want_acc, want_m2 = mc.add(acc, m2, frame)
    assert mc.capped(frame).sum() == 3 and (mc.luma(frame) < 0).any()
    assert want_m2[0, 0] == m2[0, 0] + np.uint64(2 ** 52) and want_m2[0, 1] == m2[0, 1] + np.uint64(2 ** 52) and want_m2[0, 2] == m2[0, 2] + np.uint64(2 ** 52)
    assert want_m2[0, 3] == m2[0, 3] + np.uint64((183 * 366715) ** 2)
    assert want_m2[1, 0] == want_m2[1, 1] == want_m2[1, 2] == np.uint64(2 ** 64 - 1)
    got_acc, got_m2 = acc.copy(), m2.copy()
    hk.moments_add(got_acc, got_m2, frame)
    assert np.array_equal(got_acc, want_acc) and np.array_equal(got_m2, want_m2)
    # python integers, pixel by pixel
    for x, y in ((0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (5, 5), (1, 1), (36, 10)):
        r, g, b = (int(v) for v in frame[x, y])
        yy = 54 * r + 183 * g + 19 * b
        yc = min(max(yy, -2 ** 26), 2 ** 26)
        assert int(got_m2[x, y]) == min(int(m2[x, y]) + yc * yc, 2 ** 64 - 1), (x, y)


def check_error(hk, acc, hist, m2, st, W, H, n, tol):
    gw, gh = dc.grid(st, W, H)
    sig, res = hk.error(acc, hist, m2, st, n, tol)
    wsig, wres = mc.error(acc, hist, m2, gw, gh, n, tol)
    assert res == wres, (res, wres)
    assert dc.same_bits(sig, wsig), int((dc.bits(sig) != dc.bits(wsig)).sum())
    assert sum(res["bins"]) == res["estimated"] <= res["pixels"] == gw * gh
    assert res["above"] <= res["estimated"]
    assert not sig[gh:].any() and not sig[:, gw:].any()
    return sig, res


def test_error_equals_the_restatement(hk, orc, synth, tmp_path):
    rng = np.random.default_rng(8)
    for name, path, st, bg, W, H in scene_cases(orc, synth, tmp_path):
        gw, gh = dc.grid(st, W, H)
        acc, m2, _, kept = accumulate(hk, hk.Scene(path, ""), st, bg, W, H, 16, checkpoints=(1, 2, 16))
        hist = np.zeros((W, H), np.int32)
        hist[:gw, :gh] = rng.integers(0, 4, size=(gw, gh))
        for n in (0, 1, 2, 16):
            a, m = kept[max(n, 1)]
            for h in (None, hist):
                for tol in (0.0, 0.75, 1e9):
                    sig, res = check_error(hk, a, h, m, st, W, H, n, tol)
                hn = n if h is None else h[:gw, :gh] + n
                assert res["estimated"] == int(np.sum(np.broadcast_to(hn, (gw, gh)) >= 2)), (name, n)
                if h is None and n < 2:
                    assert res["estimated"] == 0 and res["sum_var_q16"] == 0 and not sig.any()
        # 16 frames, no history: the noisy pixels are estimated as noisy, a huge tolerance is above nothing, 0 below every noisy pixel
        sig, res = check_error(hk, acc, None, m2, st, W, H, 16, 0.0)
        assert res["estimated"] == gw * gh and res["above"] == int((sig > 0).sum()) > 0, name
        assert check_error(hk, acc, None, m2, st, W, H, 16, 1e9)[1]["above"] == 0
        assert len(set(np.nonzero(res["bins"])[0])) >= 3, (name, res["bins"])
        print("error %s 16 frames: %s" % (name, res))
    # half resolution: pixels outside the grid have sigma 0 and are not counted
    half = st.copy()
    half[11] = 2
    sig, res = check_error(hk, acc, None, m2, half, W, H, 16, 0.5)
    assert res["pixels"] == (W // 2 // 8 * 8) * (H // 2 // 8 * 8)
    # a saturated plane, negative sums and a sum beyond 2^53 stay finite and equal
    big_acc = np.full((W, H, 3), 2 ** 31 - 1, np.int32)
    big_acc[::2] = -2 ** 31
    big_m2 = np.full((W, H), 2 ** 64 - 1, np.uint64)
    big_m2[:, ::2] = 0
    big_acc[:, 1::4] = 0                                # M2 = 2^64 - 1 over sums of 0: the largest sigma there is
    sig, res = check_error(hk, big_acc, None, big_m2, st, W, H, 2, 1.0)
    assert np.isfinite(sig).all() and res["bins"][15] > 0 and res["bins"][0] > 0
    with pytest.raises(RuntimeError):
        hk.error(acc, None, m2, st, -1, 0.0)
    for tol in (-0.5, float("nan")):
        with pytest.raises(RuntimeError):
            hk.error(acc, None, m2, st, 4, tol)


def test_carry(hk, orc, synth, tmp_path):
    rng = np.random.default_rng(12)
    name, path, st, bg, W, H = scene_cases(orc, synth, tmp_path)[0]
    scene = hk.Scene(path, "")
    g = scene.aov(st, W, H)
    gw, gh = dc.grid(st, W, H)
    acc, m2, _, _ = accumulate(hk, scene, st, bg, W, H, 6)
    # an identity view carries M2 unchanged (and the sums and the history as before); masked pixels (here: the sky) start again at 0
    ok = rc.allowed(g["material"], dict(rc.DEFAULTS, sky=0)).T          # [gw, gh]
    acc_to, hist_to, counts, m2_to = hk.reproject(acc, None, 6, st, st, g, g, m2=m2, sky=0)
    plain = hk.reproject(acc, None, 6, st, st, g, g, sky=0)
    assert np.array_equal(acc_to, plain[0]) and np.array_equal(hist_to, plain[1]) and counts == plain[2]
    assert np.array_equal(m2_to[:gw, :gh][ok], m2[:gw, :gh][ok]) and not m2_to[:gw, :gh][~ok].any() and ok.any() and (~ok).any()
    assert not m2_to[gw:].any() and not m2_to[:, gh:].any()
    ok = rc.allowed(g["material"], rc.DEFAULTS).T
    # cnt > max_history: python big integers, M2 * mh // cnt; values up to 2^64 - 1
    m2r = m2.copy()
    m2r[:gw:3] = rng.integers(2 ** 63, 2 ** 64 - 1, size=m2r[:gw:3].shape, dtype=np.uint64)
    m2r[0, 0] = 2 ** 64 - 1
    hist = np.zeros((W, H), np.int32)
    hist[:gw, :gh] = rng.integers(0, 70000, size=(gw, gh))
    for frames, mh, h in ((6, 4, None), (40, 8, None), (3, 5, hist), (1, 65535, hist), (9, 32, hist)):
        _, hist_to, _, m2_to = hk.reproject(acc, h, frames, st, st, g, g, m2=m2r, max_history=mh)
        cnt = (0 if h is None else h.astype(np.int64)) + frames + np.zeros((W, H), np.int64)
        assert np.array_equal(m2_to[:gw, :gh][ok], mc.carry(m2r, cnt, mh)[:gw, :gh][ok]), (frames, mh)
        xs, ys = np.nonzero(ok)
        for i in rng.choice(len(xs), 200, replace=False):
            x, y = xs[i], ys[i]
            c = int(cnt[x, y])
            assert int(m2_to[x, y]) == (int(m2r[x, y]) if c <= mh else int(m2r[x, y]) * mh // c), (frames, mh, x, y)
    # a moved view: the plane goes where the sums go
    st_b = rc.moves(st)["sideways"]
    gb = scene.aov(st_b, W, H)
    acc_to, hist_to, counts, m2_to = hk.reproject(acc, None, 6, st, st_b, g, gb, m2=m2, max_history=4)
    cam_a, cam_b = hk.camera_block(st, W, H), hk.camera_block(st_b, W, H)
    _, _, wcounts, info = rc.reproject(acc, None, 6, cam_a, cam_b, g, gb, gw, gh, max_history=4)
    v = (info["cls"] == 0).T
    assert counts == wcounts and 0 < v.sum() < gw * gh
    assert np.array_equal(m2_to[:gw, :gh][v], mc.carry(m2[info["qx"].T[v], info["qy"].T[v]], np.full(int(v.sum()), 6), 4)) and not m2_to[:gw, :gh][~v].any()
    # scaling sums and squares by the same factor keeps M2 / n - (S1 / n)^2, up to the integer truncation: |M2'/mh - M2/n| <= 1/mh and each
    # channel of the sums is off by less than 1, so |S1'/mh - S1/n| < 256/mh
    n, mh = 6, 4
    S1, S1s = mc.luma(acc), mc.luma(acc_to)
    px, py = np.nonzero(v)
    for i in rng.choice(len(px), 300, replace=False):
        x, y = int(px[i]), int(py[i])
        qx, qy = int(info["qx"].T[x, y]), int(info["qy"].T[x, y])
        before = Fraction(int(m2[qx, qy]), n) - Fraction(int(S1[qx, qy]), n) ** 2
        after = Fraction(int(m2_to[x, y]), mh) - Fraction(int(S1s[x, y]), mh) ** 2
        mean = abs(Fraction(int(S1[qx, qy]), n))
        assert abs(after - before) <= Fraction(1, mh) + 2 * mean * Fraction(256, mh) + Fraction(256, mh) ** 2, (x, y)


def test_denoise_variance(hk, orc, synth, tmp_path):
    rng = np.random.default_rng(14)
    for name, path, st, bg, W, H in scene_cases(orc, synth, tmp_path)[:2]:
        scene = hk.Scene(path, "")
        a = scene.aov(st, W, H)
        g = (a["normal"], a["albedo"], a["depth"], a["material"])
        gw, gh = dc.grid(st, W, H)
        acc, m2, _, _ = accumulate(hk, scene, st, bg, W, H, 5)
        hist = np.zeros((W, H), np.int32)
        hist[:gw, :gh] = rng.integers(0, 3, size=(gw, gh))
        for sw in ({}, {"demodulate": 0}, {"iterations": 2, "material_stop": 0}):
            # option 0 (no plane handed over) is the denoiser as it was, bit for bit
            f0, r0 = hk.denoise(acc, st, 5, *g, **sw)
            w0, _ = dc.denoise(acc, st, 5, *g, **sw)
            assert dc.same_bits(f0, w0), (name, sw)
            for n, h in ((5, None), (3, None), (2, hist), (4, hist)):
                f1, r1 = hk.denoise(acc, st, n, *g, hist=h, m2=m2, **sw)
                w1, wr1, temporal = mc.denoise(acc, st, n, *g, m2=m2, hist=h, **sw)
                assert dc.same_bits(f1, w1) and np.array_equal(r1, wr1), (name, sw, n)
                spatial, _ = hk.denoise(acc, st, n, *g, hist=h, **sw)
                if n == 3 and h is None:                # nobody has four samples: the spatial bits
                    assert not temporal.any() and dc.same_bits(f1, spatial), (name, sw)
                else:
                    assert temporal.any() and not dc.same_bits(f1, spatial), (name, sw, n)
                if h is not None and n == 2:            # 2 + hist in 2 .. 4: only some pixels are temporal
                    assert (~temporal).any()


def test_struct_layout_and_surface(tmp_path):
    import dogeray_amd as dr
    src = tmp_path / "layout.c"
    fields = ["pixels", "estimated", "above", "sum_var_q16", "bins"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dogeray_amd.h"\nint main(void) {\n  printf("%zu", sizeof(dr_error_result));\n' +
                   "".join('  printf(" %%zu", offsetof(dr_error_result, %s));\n' % n for n in fields) + "  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got[0] == ctypes.sizeof(dr.DrErrorResult) == 8 * 20
    assert [f[0] for f in dr.DrErrorResult._fields_] == fields
    assert got[1:] == [getattr(dr.DrErrorResult, n).offset for n in fields]
    for sym in ("dr_accum_error", "dr_accum_moments_read", "dr_accum_moments_device_ptr"):
        assert sym in dr.API_SYMBOLS and getattr(dr.lib(), sym)
    for m in ("accum_moments", "error", "render_until"):
        assert callable(getattr(dr.Context, m))
    assert callable(dr.ProgressiveRenderer.run_until)
    r = {"pixels": 1000, "estimated": 990, "above": 0}
    assert dr.Context.converged(r, 10) and not dr.Context.converged(r, 9) and not dr.Context.converged(dict(r, above=1), 10)
    assert dr.lib().dr_abi_version() == 2
    hdr = open(os.path.join(ROOT, "include", "dogeray_amd.h")).read()
    assert '"moments"' in hdr and '"denoise_variance"' in hdr
    out = subprocess.run([os.path.join(ROOT, "dogeray_amd", "bin", "dogeray"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--until-sigma" in out.stderr and "--max-frames" in out.stderr and "--sigma-out" in out.stderr
