"""The camera rays' grazing certificate on the GPU (option camera_cert).  Only the lean build and the counting build carry it (the
work-sharing build of short launches keeps the scene's margin), and a single-frame launch of a view not seen before computes no mask; so every render
here forces the lean build (coop_tiles_per_wave = 0) and renders at least two frames per launch.  Frames must be identical to camera_cert = 0 and to the
oracle; the counting build must walk fewer records with the certificate; the device's tile mask must equal the host build's (cert_leaf, the same
source) bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
from test_gpu_aov import _scaled_rts      # hf_small scaled down: its triangles enter the wide tree with their own bounds

pytestmark = pytest.mark.gpu

SEED, STRIDE = 5, 1000003


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1
    return dogeray_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


@pytest.fixture(scope="module")
def ctx(dr, synth):          # synth first: the generated scenes exist before this process touches the GPU
    c = dr.Context(0)
    c.set_option("coop_tiles_per_wave", 0)      # every launch runs the lean build (six waves per SIMD), the build that carries the certificate
    yield c
    c.close()


@pytest.fixture(scope="module")
def hf10(synth, tmp_path_factory):
    return _scaled_rts(os.path.join(synth["dir"], "hf_small.rts"), str(tmp_path_factory.mktemp("cert") / "hf10.rts"), 0.1)


def _render(ctx, st, W, H, bg, cert, frames=2, seed=SEED, counters=False):
    ctx.set_option("camera_cert", cert)
    ctx.enable_counters(counters)
    ctx.stats_reset()
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, seed, STRIDE, frames)
    out = ctx.accum_read().copy()
    stats = ctx.stats()
    flagged = ctx.get_option("cert_flagged_permille")
    ctx.enable_counters(False)
    return out, stats, flagged


def _view(dr, s, lift=None, focus=20.0):
    """The scene's camera with the focus distance (= |d| of a camera ray) as long as the bench view's, optionally the eye lowered to just above the
    target (the hill backs seen edge-on)"""
    st = dr.pack_settings13(s, 1, spp=1)
    st[7] = np.float32(focus)
    if lift is not None: st[1] = st[4] + np.float32(lift)
    return st


def test_grazing_view_lean_and_counting_builds_match_the_oracle(dr, orc, ctx, hf10):
    sc = dr.Scene.load(hf10, ""); sc.build_bvh()
    ctx.upload(sc)
    assert ctx.get_option("wide_own_bounds") > 0
    s = sc.settings()
    st = _view(dr, s, 0.3)
    W, H = 320, 192
    os_ = orc.Scene(hf10, None); os_.build_bvh()
    ref = sum(os_.render(st, W, H, s.background, SEED + STRIDE * k, nthreads=8)[0].astype(np.int64) for k in range(2))
    on, _, flagged = _render(ctx, st, W, H, s.background, 1)
    off, _, none = _render(ctx, st, W, H, s.background, 0)
    print("grazing view: %d per mille of the tiles flagged" % flagged)
    assert 0 < flagged < 1000, flagged                  # certified and flagged tiles both occur
    assert none == -1
    assert np.array_equal(on, off)
    assert np.array_equal(on.astype(np.int64), ref)
    # counting build: the same frames, and fewer records per ray with the certificate (the bit is read and the factor applied)
    con, son, _ = _render(ctx, st, W, H, s.background, 1, counters=True)
    coff, soff, _ = _render(ctx, st, W, H, s.background, 0, counters=True)
    assert np.array_equal(con, on) and np.array_equal(coff, on)
    assert son["rays"] == soff["rays"]
    print("counting build: %.3f records per ray with the certificate, %.3f without" % (son["node_visits"] / son["rays"], soff["node_visits"] / soff["rays"]))
    assert son["node_visits"] < soff["node_visits"]
    ctx.set_option("camera_cert", 1)


def test_device_mask_equals_the_host_builds(dr, ctx, hf10):
    import host_kernel
    L = host_kernel.lib()
    sc = dr.Scene.load(hf10, ""); sc.build_bvh()
    ctx.upload(sc)
    s = sc.settings()
    W, H = 320, 192
    h = L.hk_scene_load(hf10.encode(), b"")
    assert h, L.hk_last_error()
    try:
        mu = np.zeros(3, np.float32)
        assert L.hk_wide_mu(h, mu.ctypes.data) == ctx.get_option("wide_own_bounds")
        checked = 0
        for lift, aperture, factor in ((None, None, 40), (0.03, 0.02, 10), (0.3, None, 160), (0.1, 0.1, 40), (None, 0.1, 1)):
            st = _view(dr, s, lift)
            if aperture is not None: st[6] = np.float32(aperture)      # a wide lens: the tile projection's lens term
            ctx.set_option("cert_factor", factor)
            _render(ctx, st, W, H, s.background, 1)
            dev = ctx.cert_mask()
            out = np.zeros(8, np.int64)
            host = np.zeros((W // 8) * (H // 8) // 32 + 3, np.uint32)
            assert L.hk_cert_check(h, st.ctypes.data, W, H, C.c_double(1e-4 * factor), C.c_float(float(mu[0])), 0, 1, out.ctypes.data, host.ctypes.data) == 0, L.hk_last_error()
            ntiles = (W // 8) * (H // 8)
            nwords = (ntiles + 31) // 32
            want = host[:nwords].copy()
            if host[nwords]: want[:] = 0xffffffff
            if ntiles % 32: want[-1] &= np.uint32((1 << (ntiles % 32)) - 1)
            assert len(dev) == nwords and np.array_equal(dev, want), (lift, aperture, factor)
            assert int(np.unpackbits(dev.view(np.uint8)).sum()) == out[4]
            print("lift %s aperture %s a_star %g: %d of %d tiles flagged, device mask = host mask" % (lift, aperture, 1e-4 * factor, out[4], ntiles))
            checked += 1
        assert checked == 5
    finally:
        L.hk_scene_free(h)
        ctx.set_option("cert_factor", 40)


def test_moving_camera_recomputes_the_mask(dr, ctx, hf10):
    sc = dr.Scene.load(hf10, ""); sc.build_bvh()
    ctx.upload(sc)
    s = sc.settings()
    W, H = 320, 192
    seen = set()
    for k in range(6):
        st = _view(dr, s, 0.02 + 0.1 * k)
        st[0] += np.float32(0.03 * k)
        on, _, flagged = _render(ctx, st, W, H, s.background, 1, seed=11 + k)
        assert flagged >= 0, k                          # a launch of two frames computes the new view's mask
        seen.add(flagged)
        off, _, _ = _render(ctx, st, W, H, s.background, 0, seed=11 + k)
        assert np.array_equal(on, off), k
    assert len(seen) > 1                                # a new view, a new mask
    ctx.set_option("camera_cert", 1)


@pytest.mark.parametrize("scale", [0.2, 0.1, 0.02])
def test_fuzz_slice_option_drawn_per_scene(dr, ctx, synth, tmp_path, scale):
    rng = np.random.default_rng(int(scale * 100))
    path = _scaled_rts(os.path.join(synth["dir"], "hf_small.rts"), str(tmp_path / "hf_scaled.rts"), scale)
    sc = dr.Scene.load(path, ""); sc.build_bvh()
    ctx.upload(sc)
    assert ctx.get_option("wide_own_bounds") > 0
    s = sc.settings()
    W, H = 160, 96
    used = 0
    for k in range(6):
        st = dr.pack_settings13(s, 1, spp=1)
        st[0:3] = st[3:6] + (st[0:3] - st[3:6]) * np.float32(rng.uniform(0.3, 1.5))
        st[1] = st[4] + np.float32(rng.uniform(0.05, 2.0) * scale)
        st[7] = np.float32(st[7] * rng.choice([1.0, 10.0]))              # |d| of a camera ray: the scene's focus distance or ten times it
        st[6] = np.float32(rng.choice([0.0, 0.01, 0.1]) * st[7])          # lens up to a tenth of the focus distance
        factor = int(rng.choice([1, 10, 40, 400]))
        cert = int(rng.integers(0, 2)) if k > 0 else 1
        ctx.set_option("cert_factor", factor)
        a, _, flagged = _render(ctx, st, W, H, s.background, cert, seed=100 + k)
        if cert:
            assert flagged >= 0, (scale, k)             # the certificate was in use
            used += 1
        b, _, _ = _render(ctx, st, W, H, s.background, 0, seed=100 + k)
        assert np.array_equal(a, b), (scale, k, cert, factor)
    assert used >= 1
    ctx.set_option("cert_factor", 40); ctx.set_option("camera_cert", 1)
