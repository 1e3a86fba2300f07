"""The camera rays' grazing certificate (option camera_cert) on the host build of the kernel's own code:
 * the lemma with a certificate: a ray with |a^| >= A for its triangle keeps every accepted hit inside the own bounds widened by the margin whose
   |d|-proportional part is scaled by 1e-4 / A (the adversarial sampler of test_margin_lemma.py, |d| from 1 to 30);
 * the per-view mask is conservative: camera rays built by camera_prepare / camera_finish through random points of padded boxes have |a^| >= a_star
   when the box's triangle is certified, and land in a flagged tile when it is not (device_cert.hpp cert_leaf, tools/host_kernel.cpp hk_cert_check)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_margin_lemma import _cases      # the adversarial sampler, reused as it is


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.mark.parametrize("dlen", [1.0, 4.0, 12.0, 30.0])
def test_certified_hits_stay_inside_the_scaled_margin(hk, dlen):
    L = hk.lib()
    rng = np.random.default_rng(int(dlen * 7) + 11)
    accepted = 0
    worst = 0.0
    for rep in range(3):
        o, d, v0, e1, e2 = [np.ascontiguousarray(a, np.float32) for a in _cases(rng, 60000, 0.03, 30.0, dlen, 15.0)]
        n = len(o)
        t = np.empty(n, np.float32)
        L.hk_tri_hit(n, o.ctypes.data, d.ctypes.data, v0.ctypes.data, e1.ctypes.data, e2.ctypes.data, t.ctypes.data)
        a64 = np.abs(np.einsum("ij,ij->i", d.astype(np.float64), np.cross(e1.astype(np.float64), e2.astype(np.float64))))
        A = a64 * (1 - 1e-9)                        # the certificate each pair satisfies (its own |a^|, from below)
        idx = np.nonzero((t > 0) & (t < 10000) & (A >= 1e-4))[0]
        o64, d64, v64, p64, q64 = [z[idx].astype(np.float64) for z in (o, d, v0, e1, e2)]
        x = o64 + t[idx].astype(np.float64)[:, None] * d64
        lo = np.minimum(v64, np.minimum(v64 + p64, v64 + q64)); hi = np.maximum(v64, np.maximum(v64 + p64, v64 + q64))
        out = np.maximum(np.maximum(lo - x, x - hi), 0).max(axis=1)
        n1 = np.linalg.norm(p64, axis=1); n2 = np.linalg.norm(q64, axis=1); nv = np.linalg.norm(v64, axis=1)
        up = lambda z: np.nextafter(np.asarray(z).astype(np.float32), np.float32(np.inf))
        E = up(n1 * n2); LL = up(n1 + n2); V = up(nv)
        one = np.empty(1, np.float32)
        for j in range(len(idx)):
            k = L.hk_cert_factor_k(float(A[idx[j]]))           # 1e-4 / A rounded up, as the context computes it for a_star
            # the kernel's wide_ray_margin with the scene's E and the certificate's factor as its last argument
            L.hk_ray_margin_k(1, o[idx[j]].ctypes.data, d[idx[j]].ctypes.data, C.c_float(max(float(E[j]), 2.0 ** -100)), C.c_float(float(LL[j])),
                              C.c_float(float(V[j])), C.c_float(k), one.ctypes.data)
            r = out[j] / float(one[0])
            assert r <= 1.0, "accepted hit %.3g outside its bounds, certified margin %.3g (|a^| %.3g, |d| %.3g)" % (out[j], one[0], A[idx[j]], np.linalg.norm(d64[j]))
            worst = max(worst, r)
        accepted += len(idx)
    assert accepted > 2000
    print("|d| ~%g: %d accepted certified hits, worst distance / certified margin %.2e" % (dlen, accepted, worst))


@pytest.mark.parametrize("a_star_units", [10, 40, 160])
def test_mask_is_conservative(hk, synth, a_star_units):
    L = hk.lib()
    h = L.hk_scene_load(os.path.join(synth["dir"], "hf_small.rts").encode(), b"")
    assert h, L.hk_last_error()
    ran = 0
    try:
        for view in range(3):
            # the scene's own camera, then two lower, grazing views
            st = np.array([0, 0, 0, 0, 0, 0, 0.005, 1, 40, 10, 1, 1, 0], np.float32)
            with open(os.path.join(synth["dir"], "hf_small.rts")) as f:
                line = [l for l in f.read().split("\n") if l.startswith("*")][0].split(",")
            st[0:3] = [float(v) for v in line[1:4]]; st[3:6] = [float(v) for v in line[5:8]]      # '*,campos,aperture,look,focus,fov,...'
            st[7] = float(line[8]); st[8] = float(line[9])
            if view > 0:
                st[1] = st[4] + 0.3 * view          # eye just above the target height: grazing
            st[6] = np.float32((0.005, 0.2, 0.6)[view])      # lens diameter: the bench's, then wide ones (the tile projection's lens term)
            out = np.zeros(8, np.int64)
            W, Hh = 320, 192
            mask = np.zeros((W // 8) * (Hh // 8) // 32 + 3, np.uint32)
            rc = L.hk_cert_check(h, st.ctypes.data, W, Hh, C.c_double(1e-4 * a_star_units), C.c_float(1e30), 200000, 7 + view, out.ctypes.data, mask.ctypes.data)
            if rc != 0:
                continue
            ran += 1
            assert out[1] == 0, "a certified box was passed by a camera ray with |a^| below a_star: %s" % out
            assert out[3] == 0, "a camera ray through a flagged box lies in an unflagged tile: %s" % out
            assert out[0] + out[2] > 1000
            print("view %d a_star %g: %d rays through certified boxes, %d through flagged ones, %d of %d tiles flagged" %
                  (view, 1e-4 * a_star_units, out[0], out[2], out[4], out[5]))
    finally:
        L.hk_scene_free(h)
    assert ran >= 2
