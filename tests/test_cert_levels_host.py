"""The graded grazing certificate (option cert_levels) on the host build of the kernel's own code (tools/host_kernel.cpp):
 * the lemma at every step of the ladder: a ray with |a^| >= a_star keeps every accepted hit inside the own bounds widened by the margin scaled by
   cert_factor_k(a_star) (the adversarial sampler of test_margin_lemma.py);
 * hk_cert_levels, the grades of a view's tiles from the same cert_leaf the device runs: its sampling check per step (no camera ray through a box of
   grade g has |a^| below step g - 1, every ray through a box lies in a tile of no higher grade), the tiles below the base step are exactly
   hk_cert_check's mask at cert_factor, and the host render with the grades is the oracle's frame and the host render without them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_margin_lemma import _cases      # the adversarial sampler, reused as it is
from test_gpu_aov import _scaled_rts      # hf_small scaled down: its triangles enter the wide tree with their own bounds
import cert_level_cases as cases

SEED = 5


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    return dogeray_amd


@pytest.mark.parametrize("cert_factor", [1, 40])
def test_every_step_of_the_ladder_keeps_accepted_hits_inside_its_margin(hk, cert_factor):
    L = hk.lib()
    rng = np.random.default_rng(cert_factor + 3)
    steps = sorted(set(cases.ladder(cert_factor)))
    seen = {a: 0 for a in steps}
    for dlen in (1.0, 12.0):
        o, d, v0, e1, e2 = [np.ascontiguousarray(a, np.float32) for a in _cases(rng, 60000, 0.03, 30.0, dlen, 15.0)]
        n = len(o)
        t = np.empty(n, np.float32)
        L.hk_tri_hit(n, o.ctypes.data, d.ctypes.data, v0.ctypes.data, e1.ctypes.data, e2.ctypes.data, t.ctypes.data)
        a64 = np.abs(np.einsum("ij,ij->i", d.astype(np.float64), np.cross(e1.astype(np.float64), e2.astype(np.float64)))) * (1 - 1e-9)
        up = lambda z: np.nextafter(np.asarray(z).astype(np.float32), np.float32(np.inf))
        for units in steps:
            a_star = 1e-4 * units
            idx = np.nonzero((t > 0) & (t < 10000) & (a64 >= a_star))[0]
            if len(idx) == 0:
                continue
            o64, d64, v64, p64, q64 = [z[idx].astype(np.float64) for z in (o, d, v0, e1, e2)]
            x = o64 + t[idx].astype(np.float64)[:, None] * d64
            lo = np.minimum(v64, np.minimum(v64 + p64, v64 + q64)); hi = np.maximum(v64, np.maximum(v64 + p64, v64 + q64))
            out = np.maximum(np.maximum(lo - x, x - hi), 0).max(axis=1)
            n1 = np.linalg.norm(p64, axis=1); n2 = np.linalg.norm(q64, axis=1)
            k = L.hk_cert_factor_k(a_star)
            oo, dd = np.ascontiguousarray(o[idx]), np.ascontiguousarray(d[idx])
            # every pair against the margin of its own triangle's E, L, V (the sharp statement), scaled by the step's factor
            m = np.empty(len(idx), np.float32)
            one = np.empty(1, np.float32)
            Ei = up(n1 * n2); Li = up(n1 + n2); Vi = up(np.linalg.norm(v64, axis=1))
            for j in range(len(idx)):
                L.hk_ray_margin_k(1, oo[j].ctypes.data, dd[j].ctypes.data, C.c_float(max(float(Ei[j]), 2.0 ** -100)), C.c_float(float(Li[j])), C.c_float(float(Vi[j])),
                                  C.c_float(k), one.ctypes.data)
                m[j] = one[0]
            assert np.all(out <= m), "step %g: an accepted hit %.3g outside its bounds, margin %.3g" % (units, (out - m).max(), m[np.argmax(out - m)])
            seen[units] += len(idx)
    print("accepted hits per step (units of 1e-4):", seen)
    assert all(v > 200 for v in seen.values()), seen


@pytest.mark.parametrize("size", cases.SIZES)
def test_grades_are_conservative_match_the_mask_and_render_the_oracles_frame(hk, dr, synth, tmp_path, size):
    from oracle import orc
    W, H = size
    ran = strong = 0
    for scale in cases.SCALES:      # (at 0.02 the 0.01 padding dwarfs the triangles: every box is grade 0, the tiles are grade 0 or see no triangle)
        path = _scaled_rts(os.path.join(synth["dir"], "hf_small.rts"), str(tmp_path / ("hf_%g.rts" % scale)), scale)
        s = dr.Scene.load(path, "").settings()
        base13 = dr.pack_settings13(s, 1, spp=1)
        hs = hk.Scene(path)
        own, mu = hs.wide_mu()
        assert own > 0
        ref = orc.Scene(path, None); ref.build_bvh()
        L = hk.lib()
        ntiles = (W // 8) * (H // 8)
        for k, name in enumerate(cases.VIEWS):
            st = cases.view(base13, name, scale)
            for cert_factor in (40, 1):
                got = hs.cert_levels(st, W, H, cert_factor, 1, float(mu[0]), 300000 if cert_factor == 40 else 20000, 7 + k)
                if got is None:
                    continue                                  # the view gives no certificate (fill_cert_view false)
                plane, c = got
                assert c["below_step"] == 0, "a camera ray through a box of grade g has |a^| below step g - 1: %s" % c
                assert c["tile_above"] == 0, "a camera ray through a box lies in a tile of a higher grade: %s" % c
                assert c["n_levels"] == 5 and c["base"] == 2 and c["tiles"] == ntiles and plane.max() <= 5
                # the tiles below the base step are the one-bit certificate's flagged tiles
                out = np.zeros(8, np.int64)
                words = np.zeros((ntiles + 31) // 32 + 2, np.uint32)
                assert L.hk_cert_check(hs.h, st.ctypes.data, W, H, C.c_double(1e-4 * cert_factor), C.c_float(float(mu[0])), 0, 1, out.ctypes.data, words.ctypes.data) == 0
                assert np.array_equal(plane <= c["base"], cases.mask_bits(words, ntiles)), (name, cert_factor)
                # the single step (cert_levels = 0) is that mask too
                one, c1 = hs.cert_levels(st, W, H, cert_factor, 0, float(mu[0]), 0, 1)
                assert c1["n_levels"] == 1 and np.array_equal(one == 0, cases.mask_bits(words, ntiles))
                if cert_factor != 40:
                    continue
                print("scale %g %dx%d %s: tiles per grade %s, rays through boxes per grade %s" % (scale, W, H, name, c["tiles_per_grade"][:6], c["rays_per_grade"][:6]))
                ran += 1
                strong += c["rays_certified"] >= 1000
                want = ref.render(st, W, H, s.background, SEED, nthreads=8)[0]
                plain, cp = hs.render(st, W, H, s.background, SEED, nthreads=8)
                graded, cg = hs.render(st, W, H, s.background, SEED, nthreads=8, level_plane=plane, cert_factor=cert_factor, graded=1)
                flat, cf = hs.render(st, W, H, s.background, SEED, nthreads=8, level_plane=one, cert_factor=cert_factor, graded=0)
                assert np.array_equal(graded, want) and np.array_equal(plain, want) and np.array_equal(flat, want), name
                assert cg["rays"] == cf["rays"] and cg["V"] <= cf["V"], (cg, cf)      # a grade's margin is never wider than the single step's
    assert ran >= 2 and strong >= 2, (ran, strong)


def test_the_option_and_the_call_are_in_the_header_and_the_binding(dr):
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    hdr = open(os.path.join(root, "include", "dogeray_amd.h")).read()
    src = open(os.path.join(root, "dogeray_amd", "csrc", "context.cpp")).read()
    assert '"cert_levels"' in hdr and '"cert_levels"' in src
    assert "int dr_stats_cert_levels(dr_context* c, uint8_t* out_bytes, int max, int* n_tiles);" in hdr
    assert "dr_stats_cert_levels" in dr.API_SYMBOLS and hasattr(dr.Context, "cert_levels")
