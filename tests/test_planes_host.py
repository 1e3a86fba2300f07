"""The inputs of tests/test_gpu_planes.py are fair -- checked without a GPU, on the host build of the device functions alone.  For every case the
GPU file runs (the tables of tests/plane_cases.py) this file asserts the conditions that make the GPU comparison mean something:

  * no NaN in a reference that is compared by bits (x86 and gfx950 give different default NaN patterns): every sigma plane and every denoised
    plane of the host build is free of NaN -- the permitted share is 0, and a case that breaks it gets another input, never a mask;
  * each edge is reached: pixels above the 2^26 luma cap and the pixel just below it uncapped, negative luma, three M2 values that stay at,
    pass and reach 2^64 - 1, bins 0 and 15 and the 2^40 cap of the fixed-point variance, all four reprojection classes over the moves (the
    sideways move of the cube gives valid and rejected pixels and, with sky = 0, masked ones; off-screen pixels come from other moves), valid pixels with cnt > max_history and with cnt <= max_history, history divisors of 0 and of 65536 and more;
  * the sums of the fused add stay inside int32 (the host build's += is signed);
  * host build == numpy / big-integer restatement on the same planes, with a history plane too."""
import os
import sys

import numpy as np
import pytest

from conftest import CUBE_SETTINGS, ROOT, SCENES, with_settings
import denoise_checks as dc
import moments_checks as mc
import plane_cases as pc
import reproject_checks as rc

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.fixture(scope="module")
def cube(hk, tmp_path_factory):
    """(path, host-build scene, oracle scene, settings13, the scene's own background)"""
    from oracle import orc
    path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path_factory.mktemp("planes") / "cube.rts"), CUBE_SETTINGS)
    ref = orc.Scene(path, None)
    ref.build_bvh()
    s = ref.settings()
    return path, hk.Scene(path, ""), ref, orc.settings13(s, 1), s.background


def test_generators():
    for W, H in pc.SIZES:
        for make in (pc.acc_wide, pc.acc_mixed):
            a = make(W, H)
            assert a.dtype == np.int32 and a.shape == (W, H, 3) and np.array_equal(a, make(W, H)) and (a < 0).any() and (a > 0).any()
        wide, mixed = pc.acc_wide(W, H), pc.acc_mixed(W, H)
        assert wide.max() > 2 ** 30 and wide.min() < -2 ** 30
        assert (~mixed.any(axis=2)).any() and np.abs(mixed.astype(np.int64)).max() > 2 ** 24
        h = pc.hist(W, H)
        assert h.dtype == np.int32 and h.shape == (W, H) and not h[::5].any() and h.min() == 0 and h.max() >= 65536 and h.max() < 70000
        m = pc.m2_wide(W, H, mixed)
        assert m.dtype == np.uint64 and m.shape == (W, H)
        assert (m[:, 1::7] >= np.uint64(2 ** 63)).all() and (m[:, 3::7] == np.uint64(pc.U64_MAX)).all() and not m[:, 5::7].any()
        assert mixed[:, 5::7].any(axis=2).all()                     # ... zero over non-zero sums
        assert (m[:, 0::7] < np.uint64(2 ** 63)).any() and (m[:, 0::7] >= np.uint64(2 ** 53)).any()
    assert [dc.grid(np.array([0] * 11 + [1, 0], np.float32), W, H) for W, H in pc.SIZES] == [(136, 96), (32, 8), (32, 8), (8, 8)]
    assert [W * H % 4 for W, H in pc.SIZES] == [3, 2, 3, 1]
    # the restated present, pixel by pixel in Python integers
    acc, h = pc.acc_wide(*pc.TILE), pc.hist(*pc.TILE)
    for d in (0,) + pc.PRESENT_DIVIDE_BY:
        img = pc.present(acc, h, d)
        for x, y in ((0, 0), (1, 1), (5, 3), (12, 8), (7, 2)):
            n = int(h[x, y]) + d
            for k in range(3):
                v = int(acc[x, y, k])
                q = 0 if n == 0 else (abs(v) // n) * (1 if v >= 0 else -1)
                assert img[y, x, k] == min(max(q, 0), 255), (d, x, y, k)


def test_frames_reach_the_edges_of_the_conversion(hk, cube):
    """store_pixel's saturating float -> int at every background of the GPU test: the host build is the oracle, frame for frame, and the edges
    are there (the sky of the cube scene at CUBE_SETTINGS is more than half of the grid)"""
    path, scene, ref, st, _ = cube
    for W, H in pc.FRAME_SIZES:
        for bg in pc.BACKGROUNDS:
            for seed in pc.FRAME_SEEDS:
                f, _ = scene.render(st, W, H, bg, seed, nthreads=4, count=False)
                want, _ = ref.render(st, W, H, bg, seed, nthreads=4)
                assert np.array_equal(f, want), (W, H, bg, seed)
                y = mc.luma(f)
                if bg == 3000.0:
                    assert mc.capped(f).sum() > 0 and (y > 0).any()
                    if (W, H, seed) == (117, 89, 5):
                        assert mc.capped(f).sum() == 9847
                elif bg == -3000.0:
                    assert (y < 0).sum() > 0 and y.min() >= -765000 * 256
                    if (W, H, seed) == (117, 89, 5):
                        assert (y < 0).sum() == 9856 and f.min() == -765000
                elif bg in (1e7, float("inf")):
                    assert (f == pc.INT_MAX).any(axis=2).sum() > W * H // 4
                elif bg in (-1e7, float("-inf")):
                    assert (f == -2 ** 31).any(axis=2).sum() > W * H // 4
                else:                                           # NaN -> 0: a black sky
                    assert not f[0, 0].any()


def test_fused_add_inputs(hk, cube):
    path, scene, ref, st, _ = cube
    for W, H in pc.SIZES:
        frames = [scene.render(st, W, H, bg, pc.ADD_SEED + pc.STRIDE * k, nthreads=4, count=False)[0] for k, bg in enumerate(pc.ADD_BACKGROUNDS)]
        acc0, m20, sat = pc.add_inputs(W, H, frames)
        assert pc.fits_int32(acc0, frames)
        assert sum(int(mc.capped(f).sum()) for f in frames[:3]) > 0 and sum(int((mc.luma(f) < 0).sum()) for f in frames[3:]) > 0
        acc, m2 = acc0.copy(), m20.copy()
        want_acc, want_m2 = acc0, m20
        for f in frames:
            hk.moments_add(acc, m2, f)
            want_acc, want_m2 = mc.add(want_acc, want_m2, f)
            assert np.array_equal(acc, want_acc) and np.array_equal(m2, want_m2)
        assert np.array_equal(acc.astype(np.int64), acc0.astype(np.int64) + sum(f.astype(np.int64) for f in frames))
        # the three explicit values: one stays at 2^64 - 1, one passes it, one reaches it exactly with the first frame and stays
        first = mc.add(acc0, m20, frames[0])[1]
        assert all(int(first[p]) == pc.U64_MAX for p in sat) and all(int(m2[p]) == pc.U64_MAX for p in sat)
        assert int(m20[sat[2]]) + int(mc.square(frames[0])[sat[2]]) == pc.U64_MAX and int(m20[sat[2]]) < pc.U64_MAX
        # the explicit frame, which only the host build can be handed: capped pixels, the one just below the cap not, negative luma
        frame, over = pc.explicit_frame(W, H)
        acc, m2 = pc.acc_mixed(W, H, 1) // 2, pc.m2_wide(W, H) >> np.uint64(2)
        for p, v in over.items():
            m2[p] = np.uint64(v)
        want_acc, want_m2 = mc.add(acc, m2, frame)
        assert mc.capped(frame).sum() == 3 and not mc.capped(frame)[0, 3] and (mc.luma(frame) < 0).any()
        assert want_m2[0, 2] == m2[0, 2] + np.uint64(2 ** 52) and want_m2[0, 3] == m2[0, 3] + np.uint64((183 * 366715) ** 2)
        assert all(int(want_m2[p]) == pc.U64_MAX for p in over)
        hk.moments_add(acc, m2, frame)
        assert np.array_equal(acc, want_acc) and np.array_equal(m2, want_m2)
        # one frame of INT_MAX (background 1e7) into a zeroed accumulator
        f, _ = scene.render(st, W, H, 1e7, pc.ADD_SEED, nthreads=4, count=False)
        acc, m2 = np.zeros((W, H, 3), np.int32), np.zeros((W, H), np.uint64)
        hk.moments_add(acc, m2, f)
        sky = (f == pc.INT_MAX).any(axis=2)
        assert sky.any() and np.array_equal(acc, f) and (m2[sky] == np.uint64(2 ** 52)).all() and np.array_equal(m2, mc.square(f))


def test_error_inputs(hk, cube):
    st = cube[3]
    for W, H in pc.ERROR_SIZES:
        gw, gh = dc.grid(st, W, H)
        bins, capped_q, divisors = np.zeros(16, np.int64), 0, set()
        for name, acc, h, m2 in pc.error_cases(W, H):
            for n in ((2,) if name == "extreme" else pc.ERROR_DIVIDE_BY):
                for tol in pc.ERROR_TOLERANCES:
                    sig, res = hk.error(acc, h, m2, st, n, tol)
                    wsig, wres = mc.error(acc, h, m2, gw, gh, n, tol)
                    assert res == wres, (W, H, name, n, tol)
                    assert not np.isnan(sig).any() and np.isfinite(sig).all() and dc.same_bits(sig, wsig), (W, H, name, n, tol)
                bins += np.array(res["bins"])
                nn = (0 if h is None else h[:gw, :gh].astype(np.int64)) + n + np.zeros((gw, gh), np.int64)
                est, var = mc.variance(acc[:gw, :gh], m2[:gw, :gh], nn)
                capped_q += int((est & (var * 65536.0 >= float(2 ** 40))).sum())
                divisors |= {0} if (nn == 0).any() else set()
                divisors |= {65536} if (nn >= 65536).any() else set()
        assert bins[0] > 0 and bins[15] > 0 and capped_q > 0 and divisors == {0, 65536}, (W, H, bins, capped_q, divisors)


def test_reproject_inputs(hk, cube):
    path, scene, ref, st, _ = cube
    rng = np.random.default_rng(21)
    for W, H in pc.REPROJECT_SIZES:
        gw, gh = dc.grid(st, W, H)
        views = pc.reproject_views(scene, st, W, H)
        planes = pc.reproject_planes(W, H)
        ga = views["identity"][1]
        beyond = within = 0
        seen = dict.fromkeys(rc.CLASSES, 0)
        for move, (st_b, gb) in views.items():
            for frames, accname, h, params in pc.reproject_cases():
                mh = params["max_history"]
                got = hk.reproject(planes[accname], planes["hist"] if h else None, frames, st, st_b, ga, gb, m2=planes["m2"], **params)
                counts = got[2]
                assert sum(counts[k] for k in rc.CLASSES) == counts["pixels"] == gw * gh
                plain = hk.reproject(planes[accname], planes["hist"] if h else None, frames, st, st_b, ga, gb, **params)
                assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]) and counts == plain[2]
                for k in rc.CLASSES:
                    seen[k] += counts[k]
                if move == "identity":
                    b, w = pc.check_carry(rng, planes[accname], planes["hist"] if h else None, planes["m2"], frames, mh, got)
                    beyond, within = beyond + b, within + w
                if move == "sideways":
                    # A pure translation re-projects every sky pixel onto itself and the cube stays inside the view: valid and rejected
                    # pixels, masked ones with sky = 0, and none off screen -- that class comes from the look-at change and the camera that
                    # has gone past the look-at point.
                    assert counts["valid"] > 0 and counts["rejected"] > 0 and (counts["masked"] > 0) == (params.get("sky") == 0), counts
                if move == "sideways" and h and "normal_cos" not in params:           # the numpy restatement of the sums and the classes
                    ca, cb = hk.camera_block(st, W, H), hk.camera_block(st_b, W, H)
                    want = rc.reproject(planes[accname], planes["hist"], frames, ca, cb, ga, gb, gw, gh, **params)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and counts == want[2]
                    v = (want[3]["cls"] == 0).T
                    qx, qy = want[3]["qx"].T[v], want[3]["qy"].T[v]
                    cnt = planes["hist"][qx, qy].astype(np.int64) + frames
                    assert np.array_equal(got[3][:gw, :gh][v], mc.carry(planes["m2"][qx, qy], cnt, mh)) and not got[3][:gw, :gh][~v].any()
        assert all(seen[k] > 0 for k in rc.CLASSES), (W, H, seen)
        assert beyond > 0 and within > 0, (W, H, beyond, within)


def test_denoise_and_present_inputs(hk, cube):
    path, scene, ref, st, _ = cube
    d = pc.DENOISE_DIVIDE_BY
    for W, H in pc.DENOISE_SIZES:
        g = pc.denoise_guides(scene, st, W, H)
        h = pc.hist(W, H)
        gw, gh = dc.grid(st, W, H)
        assert (g[3] == -1).any() and (g[3] != -1).any()                 # sky and surface: both branches of the demodulation
        for accname, params in pc.denoise_cases():
            acc = pc.make_acc(accname, W, H)
            for hh in (None, h):
                f, rgb = hk.denoise(acc, st, d, *g, hist=hh, **params)
                assert not np.isnan(f).any(), "%d x %d %s %s history %s: %d NaN" % (W, H, accname, params, hh is not None, int(np.isnan(f).sum()))
                assert f[:gh, :gw].any() and not f[gh:].any() and not f[:, gw:].any()
        # host build == restatement with a history plane on acc_mixed (the restatement used to swallow hist= and ignore it)
        acc = pc.acc_mixed(W, H)
        for params in ({}, {"demodulate": 0}, {"iterations": 1}):
            f, rgb = hk.denoise(acc, st, d, *g, hist=h, **params)
            wf, wrgb = dc.denoise(acc, st, d, *g, hist=h, **params)
            assert dc.same_bits(f, wf) and np.array_equal(rgb, wrgb), (W, H, params)
            assert not dc.same_bits(f, hk.denoise(acc, st, d, *g, **params)[0])
        f0, rgb0 = hk.denoise(acc, st, d, *g, hist=h, iterations=0)
        w0, wrgb0 = dc.denoise(acc, st, d, *g, hist=h, iterations=0)
        assert dc.same_bits(f0, w0) and np.array_equal(rgb0, wrgb0)
        inside = np.zeros((H, W, 3), np.uint8)
        inside[:gh, :gw] = pc.present(acc, h, d)[:gh, :gw]
        assert np.array_equal(rgb0, inside)
        # the temporal variance over m2_wide
        m2 = pc.m2_wide(W, H)
        f, rgb = hk.denoise(acc, st, d, *g, hist=h, m2=m2)
        wf, wrgb, temporal = mc.denoise(acc, st, d, *g, m2=m2, hist=h)
        assert not np.isnan(f).any() and dc.same_bits(f, wf) and np.array_equal(rgb, wrgb) and temporal.any() and (~temporal).any(), (W, H)
        # divisors of the present: 0 (with divide_by 0, which dr_accum_present refuses) and 65536 and more
        assert (h == 0).any() and (h.astype(np.int64) + min(pc.PRESENT_DIVIDE_BY) >= 65536).any()
    with pytest.raises(TypeError):
        dc.denoise(acc, st, d, *g, history=h)
    with pytest.raises(TypeError):
        hk.denoise(acc, st, d, *g, history=h)
