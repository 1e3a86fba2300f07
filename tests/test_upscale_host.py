"""The AOV-guided upsampler without a GPU: the host build of its device functions (tools/host_kernel.cpp hk_upscale = device_upscale.hpp compiled
for the CPU) against the numpy restatement (tests/upscale_checks.py), bit for bit, with guides from the host build of the AOV kernel (hk_aov);
the block mode against the integer present, a constant image, the stops' invariances, the fallback of a pixel without a tap, the albedo coming
back at full resolution, and the C layout of dr_upscale_params."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import CUBE_SETTINGS, ROOT, SCENES, with_settings
import denoise_checks as dc
import upscale_checks as uc

sys.path.insert(0, os.path.join(ROOT, "tools"))

SWITCHES = ({}, {"demodulate": 0}, {"material_stop": 0}, {"sigma_depth": 0.0, "normal_power_log2": 0}, {"normal_power_log2": 16})
NO_TAP_CAP = 0.02          # most of the output grid the restatement's no-tap mask may cover in the stop test
# scenes and divisors over the cap with the restatement alone (matball at div 8: 7.5 % -- its spheres are a few low pixels wide there); the other
# eleven lie between 0.02 % and 1.9 %
OVER_THE_CAP = {("matball", 8)}


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


class Case:
    """One scene and size: settings13 and guides per divisor, traced once"""
    def __init__(self, hk, orc, name, path, tex, W, H):
        self.name, self.W, self.H = name, W, H
        self.settings = orc.Scene(path, tex or None).settings()
        self.orc, self.scene, self.aovs = orc, hk.Scene(path, tex), {}

    def st(self, div):
        return self.orc.settings13(self.settings, div)

    def guides(self, div):
        if div not in self.aovs:
            self.aovs[div] = self.scene.aov(self.st(div), self.W, self.H)
        return self.aovs[div]


@pytest.fixture(scope="module")
def cases(hk, orc, synth, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("upscale")
    cube = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp / "cube.rts"), CUBE_SETTINGS)
    textest = os.path.join(SCENES, "textest.rts")
    if not any(l.startswith("*") for l in open(textest)):
        textest = with_settings(textest, str(tmp / "textest.rts"), CUBE_SETTINGS)
    return [Case(hk, orc, name, path, tex, W, H) for name, path, tex, W, H in
            (("cube", cube, "", 136, 96), ("matball", os.path.join(synth["dir"], "matball.rts"), "", 120, 88),
             ("textest", textest, "", 136, 96), ("hf_small", os.path.join(synth["dir"], "hf_small.rts"), "", 160, 96))]


def random_acc(rng, W, H, gw, gh, hi=20000, negative=0.05):
    acc = np.zeros((W, H, 3), np.int32)
    acc[:gw, :gh] = rng.integers(0, hi, size=(gw, gh, 3))
    acc[:gw, :gh][rng.random((gw, gh, 3)) < negative] *= -1
    return acc


def random_hist(rng, W, H, divide_by):
    """a history plane with zeros, and a few entries whose divisor hist + divide_by is 0"""
    hist = rng.integers(0, 40, size=(W, H)).astype(np.int32)
    hist[rng.random((W, H)) < 0.3] = 0
    hist[rng.random((W, H)) < 0.01] = -divide_by
    return hist


def both(hk, c, acc, div, divide_by, **kw):
    st = c.st(div)
    return hk.upscale(acc, st, divide_by, c.guides(div), c.guides(1), **kw), uc.upscale(acc, st, divide_by, c.guides(div), c.guides(1), **kw)


def same(a, b, what):
    (f1, r1, n1), (f2, r2, n2) = a, b
    assert dc.same_bits(f1, f2), "%s: f32 differs at %d values" % (what, int((dc.bits(f1) != dc.bits(f2)).sum()))
    assert np.array_equal(r1, r2) and np.array_equal(n1, n2), what


def test_host_build_equals_the_restatement(hk, cases):
    rng = np.random.default_rng(21)
    for c in cases:
        full = c.guides(1)
        assert (full["material"] == -1).any() and (full["material"] >= 0).any(), c.name
        for div in (1, 2, 3, 4, 8):
            st = c.st(div)
            gw, gh = dc.grid(st, c.W, c.H)
            assert gw > 0 and gh > 0, (c.name, div)
            acc = random_acc(rng, c.W, c.H, gw, gh)
            hist = random_hist(rng, c.W, c.H, 9)
            for sw in SWITCHES:
                for h in (None, hist):
                    what = "%s div %d %s hist %s" % (c.name, div, sw, h is not None)
                    a, b = both(hk, c, acc, div, 9, hist=h, **sw)
                    same(a, b, what)
                    f = a[0]
                    assert np.isfinite(f).all() and not f[gh * div:].any() and not f[:, gw * div:].any(), what
                    if div == 1:
                        assert not a[2][:gh, :gw][full["material"][:gh, :gw] == -1].any(), what


def test_prefilter(hk, cases):
    rng = np.random.default_rng(22)
    for c, div, it in ((cases[0], 2, 1), (cases[1], 2, 3), (cases[3], 4, 3)):
        gw, gh = dc.grid(c.st(div), c.W, c.H)
        acc = random_acc(rng, c.W, c.H, gw, gh)
        for h in (None, random_hist(rng, c.W, c.H, 5)):
            a, b = both(hk, c, acc, div, 5, hist=h, prefilter={"iterations": it})
            same(a, b, "%s prefilter %d" % (c.name, it))
            plain = hk.upscale(acc, c.st(div), 5, c.guides(div), c.guides(1), hist=h)
            assert not dc.same_bits(plain[0], a[0]) and np.array_equal(plain[2], a[2])
    c = cases[0]
    acc = np.zeros((c.W, c.H, 3), np.int32)
    for bad in ({"prefilter": {"iterations": 0}}, {"prefilter": {"demodulate": 0}}, {"prefilter": {"iterations": 2}, "mode": uc.BLOCK},
                {"prefilter": {"iterations": 2, "demodulate": 0}, "demodulate": 1}, {"mode": 2}, {"normal_power_log2": 17}, {"sigma_depth": -1.0}):
        with pytest.raises(RuntimeError):
            hk.upscale(acc, c.st(2), 1, c.guides(2), c.guides(1), **bad)
    with pytest.raises(RuntimeError):
        hk.upscale(acc, c.st(2), 0, c.guides(2), c.guides(1))


def test_block_mode_is_the_integer_present(hk, cases):
    rng = np.random.default_rng(23)
    c = cases[0]
    for div in (1, 2, 3, 8):
        st = c.st(div)
        gw, gh = dc.grid(st, c.W, c.H)
        acc = random_acc(rng, c.W, c.H, gw, gh, hi=1 << 24)
        for divide_by in (1, 3, 255, 65535):
            for h in (None, random_hist(rng, c.W, c.H, divide_by)):
                n = np.full((c.W, c.H), divide_by, np.int64) + (0 if h is None else h)
                q = np.trunc(acc.astype(np.int64) / np.where(n == 0, 1, n)[..., None])
                present = np.clip(np.where(n[..., None] == 0, 0, q), 0, 255).astype(np.uint8).transpose(1, 0, 2)
                want = np.zeros_like(present)
                want[:gh * div, :gw * div] = np.repeat(np.repeat(present[:gh, :gw], div, axis=0), div, axis=1)
                a = hk.upscale(acc, st, divide_by, None, None, hist=h, mode=uc.BLOCK)
                b = uc.upscale(acc, st, divide_by, None, None, hist=h, mode=uc.BLOCK)
                same(a, b, (div, divide_by))
                assert np.array_equal(a[1], want) and not a[2].any(), (div, divide_by)
                if div == 1:
                    assert np.array_equal(a[1], present), divide_by
                with np.errstate(all="ignore"):
                    cq = np.where(n[..., None] == 0, np.float32(0), acc.astype(np.float32) / n.astype(np.float32)[..., None]).astype(np.float32).transpose(1, 0, 2)
                assert dc.same_bits(a[0][:gh * div, :gw * div], np.repeat(np.repeat(cq[:gh, :gw], div, axis=0), div, axis=1)), (div, divide_by)


def test_constant_image(hk, cases):
    """A constant accumulator, demodulate 0: every output pixel is that constant -- four products and three sums in float32 stay below 1e-6
    relative, 1e-5 leaves room"""
    for c in cases:
        for div in (2, 3, 4, 8):
            st = c.st(div)
            gw, gh = dc.grid(st, c.W, c.H)
            acc = np.zeros((c.W, c.H, 3), np.int32)
            acc[:gw, :gh] = (5000, 811, 12345)
            f, _, _ = hk.upscale(acc, st, 7, c.guides(div), c.guides(1), demodulate=0)
            want = np.array([5000, 811, 12345], np.float64) / 7
            got = f[:gh * div, :gw * div].astype(np.float64)
            assert np.abs(got / want - 1).max() <= 1e-5, (c.name, div)


def test_stops_are_exact(hk, cases):
    """With material_stop, new colours on the low pixels of one material leave the output bits of every full-resolution pixel of every other
    material as they were; hit pixels and misses never mix, with or without material_stop.  Asserted on the pixels outside the restatement's
    no-tap mask (a pixel without a tap shows its block, whatever that block's material), which covers at most NO_TAP_CAP of the output grid."""
    rng = np.random.default_rng(24)
    for c in cases:
        for div in (2, 4, 8):
            st = c.st(div)
            gw, gh = dc.grid(st, c.W, c.H)
            Gw, Gh = gw * div, gh * div
            low, full = c.guides(div), c.guides(1)
            m, M = low["material"], full["material"][:Gh, :Gw]
            acc = random_acc(rng, c.W, c.H, gw, gh)
            base, _, notap = uc.upscale(acc, st, 4, low, full)
            share = float(notap[:Gh, :Gw].mean())
            print("no-tap share %s div %d: %.4f" % (c.name, div, share))
            if (c.name, div) in OVER_THE_CAP:
                continue
            assert share <= NO_TAP_CAP, (c.name, div, share)
            tapped = ~notap[:Gh, :Gw]
            hbase, _, hno = hk.upscale(acc, st, 4, low, full)
            assert dc.same_bits(hbase, base) and np.array_equal(hno, notap)
            mats = [v for v in np.unique(m) if v >= 0]
            if len(mats) > 1:
                b = mats[-1]
                acc2 = acc.copy()
                sel = (m == b).T
                acc2[:gw, :gh][sel] = rng.integers(0, 20000, size=(int(sel.sum()), 3))
                f2, _, _ = hk.upscale(acc2, st, 4, low, full)
                keep = (M != b) & tapped
                assert dc.same_bits(f2[:Gh, :Gw][keep], base[:Gh, :Gw][keep]), (c.name, div)
                assert not np.array_equal(f2[:Gh, :Gw][(M == b) & tapped], base[:Gh, :Gw][(M == b) & tapped]), (c.name, div)
            for mstop in (1, 0):
                base, _, notap = hk.upscale(acc, st, 4, low, full, material_stop=mstop)
                tapped = ~notap[:Gh, :Gw]
                for changed, Changed in ((m == -1, M == -1), (m != -1, M != -1)):
                    acc2 = acc.copy()
                    acc2[:gw, :gh][changed.T] = rng.integers(0, 20000, size=(int(changed.sum()), 3))
                    f2, _, _ = hk.upscale(acc2, st, 4, low, full, material_stop=mstop)
                    keep = ~Changed & tapped
                    assert dc.same_bits(f2[:Gh, :Gw][keep], base[:Gh, :Gw][keep]), (c.name, div, mstop)


def test_a_pixel_without_a_tap_shows_its_block(hk, cases):
    rng = np.random.default_rng(25)
    c = cases[0]
    for div in (2, 4):
        st = c.st(div)
        gw, gh = dc.grid(st, c.W, c.H)
        acc = random_acc(rng, c.W, c.H, gw, gh)
        full = {k: v.copy() for k, v in c.guides(1).items()}
        hit = np.argwhere(full["material"][:gh * div, :gw * div] >= 0)
        Y, X = (int(v) for v in hit[len(hit) // 2])
        assert 99 not in np.unique(c.guides(div)["material"])
        full["material"][Y, X] = 99                       # a material no low pixel has: a thin object only the full-resolution guides see
        for fn in (hk.upscale, uc.upscale):
            f, rgb, notap = fn(acc, st, 3, c.guides(div), full)
            assert notap[Y, X]
            want = acc[X // div, Y // div].astype(np.float32) / np.float32(3)
            assert dc.same_bits(f[Y, X], want), fn
            assert np.array_equal(rgb[Y, X], np.clip(want, 0, 255).astype(np.uint8))


def test_albedo_comes_back(hk, orc, synth, tmp_path):
    """A flat-lit low accumulator acc = trunc(200 a_q 1000), divide_by 1000, on a scene whose albedo varies inside one material: where every tap
    has an albedo >= 0.1 the guided output is 200 A_P to 0.02 (the truncation gives at most 1e-3 / 0.1 on e, float rounding is two orders below)
    -- the texture is back at full resolution -- and the block fill misses that bound on the same pixels."""
    textest = os.path.join(SCENES, "textest.rts")
    if not any(l.startswith("*") for l in open(textest)):
        textest = with_settings(textest, str(tmp_path / "textest.rts"), CUBE_SETTINGS)
    W, H = 136, 96
    s = orc.Scene(textest, synth["tex"]).settings()             # the generated stand-in of the scene's testtwo.ppm
    scene = hk.Scene(textest, synth["tex"])
    full = scene.aov(orc.settings13(s, 1), W, H)
    for div in (2, 4):
        st = orc.settings13(s, div)
        low = scene.aov(st, W, H)
        gw, gh = dc.grid(st, W, H)
        Gw, Gh = gw * div, gh * div
        A, M = full["albedo"][:Gh, :Gw], full["material"][:Gh, :Gw]
        # the precondition: some material's albedo varies across the full-resolution pixels of one low pixel
        blocks = A.reshape(gh, div, gw, div, 3)
        one = (M.reshape(gh, div, gw, div) == M.reshape(gh, div, gw, div)[:, :1, :, :1]).all(axis=(1, 3)) & (M[::div, ::div] >= 0)
        spread = (blocks.max(axis=(1, 3)) - blocks.min(axis=(1, 3))).max(axis=-1)
        assert (one & (spread > 0.1)).sum() >= 20, "the albedo does not vary inside a material"
        acc = np.zeros((W, H, 3), np.int32)
        acc[:gw, :gh] = np.trunc(np.float64(200) * low["albedo"].astype(np.float64) * 1000).astype(np.int32).transpose(1, 0, 2)
        f, _, notap = hk.upscale(acc, st, 1000, low, full)
        blk, _, _ = hk.upscale(acc, st, 1000, None, None, mode=uc.BLOCK)
        # pixels all of whose (up to four) taps inside the grid have an albedo >= 0.1 in every channel
        x0, _ = uc.position(Gw, div)
        y0, _ = uc.position(Gh, div)
        ok = np.ones((Gh, Gw), bool)
        bright = low["albedo"].min(axis=-1) >= 0.1
        for j in range(2):
            for i in range(2):
                ok &= bright[np.clip(y0 + j, 0, gh - 1)[:, None], np.clip(x0 + i, 0, gw - 1)[None, :]]
        ok &= (M >= 0) & ~notap[:Gh, :Gw] & (A.min(axis=-1) > 1e-3)       # a' = 1 at or below 1e-3: nothing is multiplied back there
        assert ok.sum() >= 500, int(ok.sum())
        want = np.float64(200) * A.astype(np.float64)
        err = np.abs(f[:Gh, :Gw].astype(np.float64) - want).max(axis=-1)
        berr = np.abs(blk[:Gh, :Gw].astype(np.float64) - want).max(axis=-1)
        print("albedo div %d: %d pixels, guided error %.4f, block error %.4f" % (div, int(ok.sum()), err[ok].max(), berr[ok].max()))
        assert err[ok].max() <= 0.02, (div, float(err[ok].max()))
        assert berr[ok].max() > 0.02, (div, float(berr[ok].max()))


def test_upscale_params_layout_matches_the_header(tmp_path):
    import dogeray_amd as dr
    hdr = open(os.path.join(ROOT, "include", "dogeray_amd.h")).read()
    body = re.search(r"typedef struct dr_upscale_params \{(.*?)\} dr_upscale_params;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int|float)\s+(\w+)\s*;", body)
    assert [f[1] for f in fields] == [f[0] for f in dr.DrUpscaleParams._fields_] == list(uc.DEFAULTS)
    assert [f[0] for f in fields] == ["float" if t is ctypes.c_float else "int" for _, t in dr.DrUpscaleParams._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dogeray_amd.h"\nint main(void) {\n  printf("%zu", sizeof(dr_upscale_params));\n' +
                   "".join('  printf(" %%zu", offsetof(dr_upscale_params, %s));\n' % n for _, n in fields) +
                   '  printf(" %d %d", DR_UPSCALE_BLOCK, DR_UPSCALE_GUIDED);\n  return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got[0] == ctypes.sizeof(dr.DrUpscaleParams)
    assert got[1:-2] == [getattr(dr.DrUpscaleParams, n).offset for _, n in fields]
    assert got[-2:] == [dr.UPSCALE_BLOCK, dr.UPSCALE_GUIDED] == [uc.BLOCK, uc.GUIDED]
    # the library's defaults are the restatement's (dr_upscale_defaults needs no GPU)
    p = dr.upscale_params()
    assert {k: getattr(p, k) for k in uc.DEFAULTS} == uc.DEFAULTS
    assert dr.lib().dr_abi_version() == 2
