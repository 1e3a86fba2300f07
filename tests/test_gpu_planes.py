"""The accumulator's kernels on the GPU over adversarial planes: the fused acc += frame, M2 += yc^2 add, dr_accum_error, dr_accum_reproject with
the history plane and the M2 carry, the a-trous denoiser in both shapes, dr_accum_present with a history plane and the plain frame add.

The planes (tests/plane_cases.py) are written into the live device planes through the *_device_ptr calls (tests/device_planes.py): sums over
the whole of int32 and of both signs, history counts of 0 and beyond 65535, M2 at and above 2^53, 2^63 and 2^64 - 1 -- what rendered frames never
give.  Frames are pushed to the edges through the render path: backgrounds of +-3000 (sky above the 2^26 luma cap, negative luma), +-1e7 and
+-inf (beyond int32, 0 * inf) and NaN.

The reference is always the host build of the same device header (tools/host_kernel.py) fed the planes READ BACK from the GPU before the call
(and the read-back is asserted equal to what was written), with the numpy / big-integer restatements (moments_checks, reproject_checks,
denoise_checks, plane_cases.present) as a second reference.  Conditions, each asserted without a GPU by tests/test_planes_host.py on these same
cases: no reference compared by bits holds a NaN (x86 and gfx950 give different default NaN patterns; the permitted share is 0); the cap, the
saturation, bins 0 and 15, the 2^40 cap, every reprojection class, cnt on both sides of max_history and divisors of 0 and >= 65536 are reached;
the fused add's sums stay inside int32.

What the API does not let through: dr_accum_present refuses divide_by 0 and dr_accum_denoise divide_by < 1 (asserted), so a divisor of 0 reaches
only dr_accum_error; a frame cannot be handed to the add, so the explicit frame pixels of test_moments_host.py stay with the host file and the
explicit M2 values are installed against the squares of the GPU's own first frame.  For the cube a sideways move gives no off-screen and
(with sky = 1) no masked pixel: all four classes are asserted over the set of moves, masked through a run with sky = 0."""
import os
import sys

import numpy as np
import pytest

from conftest import CUBE_SETTINGS, ROOT, SCENES, with_settings
import denoise_checks as dc
import device_planes as dp
import moments_checks as mc
import plane_cases as pc
import reproject_checks as rc

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))
STRIDE = pc.STRIDE
RESTORE = (("moments", 0), ("denoise_variance", 0), ("pipe_group", 8), ("denoise_tiles", 1), ("kernel", 1))


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.fixture(scope="module")
def world(dr, hk, tmp_path_factory):          # hk first: everything is compiled before this process touches the GPU
    """one Context with the cube at CUBE_SETTINGS for the whole file, and the scene for the host build and the oracle"""
    from oracle import orc
    path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path_factory.mktemp("planes") / "cube.rts"), CUBE_SETTINGS)
    ref = orc.Scene(path, None)
    ref.build_bvh()
    sc = dr.Scene.load(path, "")
    sc.build_bvh()
    c = dr.Context(0)
    c.upload(sc)
    yield {"ctx": c, "st": dr.pack_settings13(sc.settings(), 1), "host": hk.Scene(path, ""), "oracle": ref}
    c.close()


@pytest.fixture()
def ctx(world):
    c = world["ctx"]
    try:
        c.set_traversal(2)
        yield c
    finally:
        for name, value in RESTORE:
            c.set_option(name, value)
        c.enable_counters(False)
        c.set_traversal(2)


@pytest.mark.parametrize("W,H", pc.FRAME_SIZES)
def test_frames_at_the_edges_of_the_conversion(dr, world, ctx, W, H):
    """store_pixel's saturating float -> int (>= 2^31, inf, 0 * inf = NaN -> 0, a NaN background): every frame is the oracle's, through the
    persistent and the tile kernel, the counting and the plain build.  dr_render_frame refuses none of these backgrounds."""
    st = world["st"]
    for bg in pc.BACKGROUNDS:
        for seed in pc.FRAME_SEEDS:
            want, _ = world["oracle"].render(st, W, H, bg, seed, nthreads=4)
            for kernel in (1, 0):
                ctx.set_option("kernel", kernel)
                for counting in (True, False):
                    ctx.enable_counters(counting)
                    got = ctx.render_frame(st, W, H, bg, seed)
                    assert np.array_equal(got, want), "%d x %d background %r seed %d kernel %d counting %d: %d pixels differ" % (
                        W, H, bg, seed, kernel, counting, int((got != want).any(axis=2).sum()))
            if bg == 3000.0:
                assert mc.capped(want).any()
            elif bg == -3000.0:
                assert (mc.luma(want) < 0).any()
            elif abs(bg) == 1e7 or np.isinf(bg):
                assert (want == (pc.INT_MAX if bg > 0 else -2 ** 31)).any()


def _fold(hk, acc, m2, frames):
    """the host build's fused add and the restatement over these frames, asserted equal: (acc, m2, [the sums after every frame])"""
    want_acc, want_m2, totals = acc, m2, []
    acc, m2 = acc.copy(), m2.copy()
    for f in frames:
        hk.moments_add(acc, m2, f)
        want_acc, want_m2 = mc.add(want_acc, want_m2, f)
        totals.append(acc.copy())
    assert np.array_equal(acc, want_acc) and np.array_equal(m2, want_m2)
    return acc, m2, totals


def _add(ctx, path, st, W, H, bg, seeds, divide_from=1):
    """adds the frames of these seeds through one of the three paths; the presents of the submit path (else None)"""
    if path == "accumulate":
        ctx.render_accumulate(st, W, H, bg, seeds[0], STRIDE, len(seeds))
    elif path == "pipelined":
        ctx.render_accumulate_pipelined(st, W, H, bg, seeds[0], STRIDE, len(seeds))
    else:
        tickets = [ctx.pipeline_submit(st, W, H, bg, sd, present_divide_by=divide_from + k) for k, sd in enumerate(seeds)]
        return [ctx.pipeline_wait(t, want_image=True) for t in tickets]
    return None


@pytest.mark.parametrize("W,H", pc.SIZES)
def test_fused_add(dr, hk, world, ctx, W, H):
    """acc_mixed and m2_wide with the three saturating values, three frames at background 3000 (capped) and three at -3000 (negative luma)
    through render_accumulate, render_accumulate_pipelined and submit / wait, pipe_group 1 and 8: the vector path, the scalar tail (W * H % 4
    = 3, 2, 3, 1) and the all-scalar path of frames that are not 16-byte aligned inside their group.  Then one frame of INT_MAX."""
    st = world["st"]
    seeds = [pc.ADD_SEED + STRIDE * k for k in range(6)]
    frames = [ctx.render_frame(st, W, H, bg, sd) for sd, bg in zip(seeds, pc.ADD_BACKGROUNDS)]          # the GPU's own frames
    acc0, m20, sat = pc.add_inputs(W, H, frames)
    assert pc.fits_int32(acc0, frames)
    assert sum(int(mc.capped(f).sum()) for f in frames[:3]) > 0 and sum(int((mc.luma(f) < 0).sum()) for f in frames[3:]) > 0
    ctx.set_option("moments", 1)
    for group in (1, 8):
        ctx.set_option("pipe_group", group)
        for path in ("accumulate", "pipelined", "submit"):
            what = "%d x %d pipe_group %d %s" % (W, H, group, path)
            ctx.accum_reset(W, H)
            acc_in, _, m2_in = dp.install(dr, ctx, acc=acc0, m2=m20)
            want_acc, want_m2, totals = _fold(hk, acc_in, m2_in, frames)
            images = (_add(ctx, path, st, W, H, 3000.0, seeds[:3]) or []) + (_add(ctx, path, st, W, H, -3000.0, seeds[3:], divide_from=4) or [])
            acc, hist, m2 = dp.peek(ctx)
            assert np.array_equal(acc, want_acc), "%s: the sums differ at %d values" % (what, int((acc != want_acc).sum()))
            assert np.array_equal(m2, want_m2), "%s: the plane differs at %d pixels" % (what, int((m2 != want_m2).sum()))
            assert all(int(m2[p]) == pc.U64_MAX for p in sat) and not hist.any(), what
            for k, img in enumerate(images):            # the pipelined presents over sums of both signs and up to 2^31
                assert np.array_equal(img, pc.present(totals[k], np.zeros((W, H), np.int32), k + 1)), "%s: present %d" % (what, k)
    # one frame of INT_MAX (background 1e7) into a zeroed accumulator, with a plane and through the plain add
    f = ctx.render_frame(st, W, H, 1e7, pc.ADD_SEED)
    assert (f == pc.INT_MAX).any()
    zero = np.zeros((W, H, 3), np.int32)
    want_acc, want_m2, _ = _fold(hk, zero, np.zeros((W, H), np.uint64), [f])
    for moments in (1, 0):
        ctx.set_option("moments", moments)
        for path in ("accumulate", "pipelined", "submit"):
            ctx.accum_reset(W, H)
            images = _add(ctx, path, st, W, H, 1e7, [pc.ADD_SEED])
            acc, _, m2 = dp.peek(ctx)
            assert np.array_equal(acc, f) and np.array_equal(acc, want_acc), (W, H, moments, path)
            assert np.array_equal(m2, want_m2 if moments else np.zeros_like(want_m2)), (W, H, moments, path)
            assert images is None or np.array_equal(images[0], pc.present(f, np.zeros((W, H), np.int32), 1))


@pytest.mark.parametrize("W,H", pc.ERROR_SIZES)
def test_error(dr, hk, world, ctx, W, H):
    """dr_accum_error over acc_wide / acc_mixed x m2_wide x {no history, hist} and the all-extreme planes: the sigma plane's bits and every
    count equal the host build's and the restatement's"""
    st = world["st"]
    gw, gh = dc.grid(st, W, H)
    ctx.set_option("moments", 1)
    bins = np.zeros(16, np.int64)
    for name, acc, h, m2 in pc.error_cases(W, H):
        ctx.accum_reset(W, H)
        if h is not None:
            dp.history(ctx, st, W, H)
        a, hh, m = dp.install(dr, ctx, acc=acc, hist=h, m2=m2)
        assert h is not None or not hh.any()
        for n in ((2,) if name == "extreme" else pc.ERROR_DIVIDE_BY):
            for tol in pc.ERROR_TOLERANCES:
                what = "%d x %d %s divide_by %d tolerance %g" % (W, H, name, n, tol)
                got = ctx.error(st, W, H, n, tol, sigma=True)
                sig, res = hk.error(a, hh if h is not None else None, m, st, n, tol, nthreads=8)
                wsig, wres = mc.error(a, hh if h is not None else None, m, gw, gh, n, tol)
                plane = got.pop("sigma")
                assert not np.isnan(sig).any(), what
                assert got == res == wres, "%s: %s, host build %s, restatement %s" % (what, got, res, wres)
                assert dc.same_bits(plane, sig) and dc.same_bits(plane, wsig), "%s: sigma differs at %d pixels" % (what, int((dc.bits(plane) != dc.bits(sig)).sum()))
                assert ctx.error(st, W, H, n, tol) == res, what
            bins += np.array(res["bins"])
        a2, h2, m2_after = dp.peek(ctx)
        assert np.array_equal(a2, a) and np.array_equal(h2, hh) and np.array_equal(m2_after, m), name        # the call changes no plane
    assert bins[0] > 0 and bins[15] > 0, bins


@pytest.mark.parametrize("W,H", pc.REPROJECT_SIZES)
def test_reproject(dr, hk, world, ctx, W, H):
    """dr_accum_reproject over acc_wide / acc_mixed, hist and m2_wide: the signed 64-bit divide of the sums and the 64-bit divide and modulo of
    the M2 carry, for the identity and the five moves, with and without the second-moment plane: sums, history, M2 and counts equal the host
    build's; on the identity 200 random valid pixels equal Python's M2 * mh // cnt"""
    st = world["st"]
    rng = np.random.default_rng(23)
    views = pc.reproject_views(world["host"], st, W, H)
    planes = pc.reproject_planes(W, H)
    ga = views["identity"][1]
    seen = dict.fromkeys(rc.CLASSES, 0)
    beyond = within = 0
    for moments in (1, 0):
        ctx.set_option("moments", moments)
        for move, (st_b, gb) in views.items():
            for frames, accname, h, params in pc.reproject_cases():
                what = "%d x %d moments %d %s %d frames %s %s history %d" % (W, H, moments, move, frames, accname, params, h)
                ctx.accum_reset(W, H)
                if h:
                    dp.history(ctx, st, W, H)
                a, hh, m = dp.install(dr, ctx, acc=planes[accname], hist=planes["hist"] if h else None, m2=planes["m2"] if moments else None)
                assert h or not hh.any()
                counts = ctx.reproject(st, st_b, W, H, frames, **params)
                want = hk.reproject(a, hh if h else None, frames, st, st_b, ga, gb, m2=m, **params)
                acc, hist, m2 = dp.peek(ctx)
                assert counts == want[2], "%s: counts %s, host build %s" % (what, counts, want[2])
                assert np.array_equal(acc, want[0]), "%s: the sums differ at %d values" % (what, int((acc != want[0]).sum()))
                assert np.array_equal(hist, want[1]), "%s: the history differs at %d pixels" % (what, int((hist != want[1]).sum()))
                assert np.array_equal(m2, want[3] if moments else np.zeros_like(m)), "%s: the plane differs at %d pixels" % (what, int((m2 != want[3]).sum()))
                for k in rc.CLASSES:
                    seen[k] += counts[k]
                if move == "identity" and moments:
                    b, w = pc.check_carry(rng, a, hh if h else None, m, frames, params["max_history"], (acc, hist, counts, m2))
                    beyond, within = beyond + b, within + w
    assert all(seen[k] > 0 for k in rc.CLASSES), seen
    assert beyond > 0 and within > 0, (beyond, within)


@pytest.mark.parametrize("W,H", pc.DENOISE_SIZES)
def test_present_and_denoise(dr, hk, world, ctx, W, H):
    """dr_accum_present and the denoiser (lattice and per-pixel shape) over synthetic sums with and without a history plane: negative sums,
    sums up to 2^31, divisors of five digits; 13 x 9 is a single 8 x 8 tile under a-trous steps up to 512.  Bit for bit the host build."""
    st = world["st"]
    d = pc.DENOISE_DIVIDE_BY
    g = pc.denoise_guides(world["host"], st, W, H)
    gw, gh = dc.grid(st, W, H)
    for with_hist in (True, False):
        for accname in ("mixed", "wide"):
            ctx.set_option("moments", 0)
            ctx.accum_reset(W, H)
            if with_hist:
                dp.history(ctx, st, W, H)
            a, hh, _ = dp.install(dr, ctx, acc=pc.make_acc(accname, W, H), hist=pc.hist(W, H) if with_hist else None)
            assert with_hist or not hh.any()
            for div in pc.PRESENT_DIVIDE_BY:
                assert np.array_equal(ctx.accum_present(div), pc.present(a, hh, div)), (W, H, accname, with_hist, div)
            with pytest.raises(dr.DogerayError):                    # divide_by 0 is refused, with a history plane too
                ctx.accum_present(0)
            with pytest.raises(dr.DogerayError, match="divide_by"):
                ctx.denoise(st, W, H, 0)
            for name, params in pc.denoise_cases():
                if name != accname:
                    continue
                want = hk.denoise(a, st, d, *g, hist=hh if with_hist else None, nthreads=8, **params)
                assert not np.isnan(want[0]).any()
                for tiles in (1, 0):
                    what = "%d x %d %s history %d %s tiles %d" % (W, H, accname, with_hist, params, tiles)
                    ctx.set_option("denoise_tiles", tiles)
                    rgb, f = ctx.denoise(st, W, H, d, out="both", **params)
                    assert dc.same_bits(f, want[0]), "%s: f32 differs at %d values" % (what, int((dc.bits(f) != dc.bits(want[0])).sum()))
                    assert np.array_equal(rgb, want[1]), what
                if accname == "mixed" and params in ({}, {"demodulate": 0}, {"iterations": 1}):         # the restatement
                    wf, wrgb = dc.denoise(a, st, d, *g, hist=hh if with_hist else None, **params)
                    assert dc.same_bits(want[0], wf) and np.array_equal(want[1], wrgb), (W, H, with_hist, params)
            ctx.set_option("denoise_tiles", 1)
            # iterations 0 is dr_accum_present inside the grid; outside it the denoiser writes 0 and the present divides the (here non-zero) sums
            r0, p0 = ctx.denoise(st, W, H, d, iterations=0), ctx.accum_present(d)
            assert np.array_equal(r0[:gh, :gw], p0[:gh, :gw]) and not r0[gh:].any() and not r0[:, gw:].any(), (W, H, accname, with_hist)
            f0 = ctx.denoise(st, W, H, d, out="f32", iterations=0)
            assert dc.same_bits(f0, hk.denoise(a, st, d, *g, hist=hh if with_hist else None, iterations=0)[0])
            if accname == "mixed":
                # the presents of two pipelined frames on top of these sums (the plain frame add: no second-moment plane)
                seeds = [101, 101 + STRIDE]
                tickets = [ctx.pipeline_submit(st, W, H, 3000.0, sd, present_divide_by=k + 2) for k, sd in enumerate(seeds)]
                images = [ctx.pipeline_wait(t, want_image=True) for t in tickets]
                total = a.astype(np.int64)
                for k, sd in enumerate(seeds):
                    total = total + ctx.render_frame(st, W, H, 3000.0, sd)
                    assert np.array_equal(images[k], pc.present(total, hh, k + 2)), (W, H, with_hist, k)
                assert np.array_equal(ctx.accum_read(), total) and np.array_equal(ctx.accum_history(), hh)
    # the temporal variance (option denoise_variance) over m2_wide: (double) M2 beyond 2^53, the ss > 0 clamp
    ctx.set_option("moments", 1)
    ctx.set_option("denoise_variance", 1)
    ctx.accum_reset(W, H)
    dp.history(ctx, st, W, H)
    a, hh, m = dp.install(dr, ctx, acc=pc.acc_mixed(W, H), hist=pc.hist(W, H), m2=pc.m2_wide(W, H))
    want = hk.denoise(a, st, d, *g, hist=hh, m2=m, nthreads=8)
    wf, wrgb, temporal = mc.denoise(a, st, d, *g, m2=m, hist=hh)
    assert not np.isnan(want[0]).any() and dc.same_bits(want[0], wf) and temporal.any()
    for tiles in (1, 0):
        ctx.set_option("denoise_tiles", tiles)
        rgb, f = ctx.denoise(st, W, H, d, out="both")
        assert dc.same_bits(f, want[0]) and np.array_equal(rgb, want[1]), (W, H, tiles)
    assert not dc.same_bits(want[0], hk.denoise(a, st, d, *g, hist=hh, nthreads=8)[0])
