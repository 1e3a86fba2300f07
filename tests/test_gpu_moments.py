"""The second-moment plane on the GPU (option "moments", dr_accum_error / Context.error, Context.render_until, ProgressiveRenderer.run_until,
dogeray --until-sigma / --sigma-out): the plane through every frame-adding path against the host build of the same device functions
(tools/host_kernel.cpp) fed with the GPU's own frames, the sums against a context without a plane, the noise estimate and the reprojected plane bit
for bit against the host build, the estimate's calibration against a long mean, the convergence stop, the denoiser's temporal variance, the
errors, the full-size scene and the command line."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import CUBE_SETTINGS, ROOT, SCENES, with_settings
import denoise_checks as dc
import moments_checks as mc
import reproject_checks as rc

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))
GUIDES = ("t", "normal", "material")
STRIDE = 1000003


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
def ctx(dr, synth):          # synth first: the generated scenes exist before this process touches the GPU
    c = dr.Context(0)
    yield c
    c.close()


@pytest.fixture()
def plane(ctx):
    """the shared context with a second-moment plane for the test, and as it was afterwards"""
    ctx.set_traversal(2)
    ctx.set_option("moments", 1)
    yield ctx
    ctx.set_option("moments", 0)
    ctx.set_option("denoise_variance", 0)
    ctx.set_option("pipe_group", 8)
    ctx.set_traversal(2)


def _cube(tmp_path):
    return with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube.rts"), CUBE_SETTINGS)


def _scene(synth, tmp_path, name):
    return os.path.join(synth["dir"], "matball.rts") if name == "matball" else _cube(tmp_path)


def _load(dr, path):
    sc = dr.Scene.load(path, "")
    sc.build_bvh()
    return sc


def _host_planes(hk, ctx, st, W, H, bg, seeds, acc=None, m2=None):
    """the sums and the plane of the GPU's own frames of these seeds, folded by the host build"""
    acc = np.zeros((W, H, 3), np.int32) if acc is None else acc.copy()
    m2 = np.zeros((W, H), np.uint64) if m2 is None else m2.copy()
    for sd in seeds:
        hk.moments_add(acc, m2, ctx.render_frame(st, W, H, bg, sd))
    return acc, m2


def _moments_ptr(dr, ctx):
    ptr, nbytes = C.c_void_p(), C.c_uint64()
    assert dr.lib().dr_accum_moments_device_ptr(ctx._h, C.byref(ptr), C.byref(nbytes)) == 0
    return ptr.value, nbytes.value


@pytest.mark.parametrize("mode", [2, 0, 1])
def test_same_plane_through_every_path(dr, hk, plane, synth, tmp_path, mode):
    ctx = plane
    N = 5
    seeds = [31 + STRIDE * k for k in range(N)]
    for name, W, H in (("cube", 136, 96), ("matball", 117, 89)):          # 117 x 89: W * H % 4 = 1, the scalar tail; frames 1 .. of a group are not 16-byte aligned
        sc = _load(dr, _scene(synth, tmp_path, name))
        ctx.upload(sc)
        ctx.set_traversal(mode)
        st, bg = dr.pack_settings13(sc.settings(), 1), sc.settings().background
        want_acc, want_m2 = _host_planes(hk, ctx, st, W, H, bg, seeds)
        assert want_m2.any()
        for group in (1, 8):
            ctx.set_option("pipe_group", group)
            got = {}
            for moments in (0, 1):
                ctx.set_option("moments", moments)
                out = {}
                ctx.accum_reset(W, H)
                ctx.render_accumulate(st, W, H, bg, seeds[0], STRIDE, N)
                out["accumulate"] = (ctx.accum_read(), ctx.accum_moments(), None)
                got[moments] = out
                if moments == 0 and group > 1 and (W * H) % 4:
                    continue                    # (the plain add has no path for unaligned frame buffers: the plane's runs are checked against the host build)
                ctx.accum_reset(W, H)
                ctx.render_accumulate_pipelined(st, W, H, bg, seeds[0], STRIDE, N)
                out["pipelined"] = (ctx.accum_read(), ctx.accum_moments(), None)
                ctx.accum_reset(W, H)
                tickets, images = [], []
                # the pipeline keeps pipe_streams + 1 = 3 groups of frames: where groups form (the wide walk's persistent kernel) all N frames are
                # one group of pipe_group 8; everywhere else every frame is a group of its own, and two are kept in flight
                window = N if (group > 1 and mode == 2) else 2
                for k in range(N):
                    tickets.append(ctx.pipeline_submit(st, W, H, bg, seeds[k], present_divide_by=k + 1))
                    if len(tickets) - len(images) >= window:
                        images.append(ctx.pipeline_wait(tickets[len(images)], want_image=True))
                while len(images) < N:
                    images.append(ctx.pipeline_wait(tickets[len(images)], want_image=True))
                out["submit"] = (ctx.accum_read(), ctx.accum_moments(), images)
            for path in ("accumulate", "pipelined", "submit"):
                what = "%s traversal %d pipe_group %d %s" % (name, mode, group, path)
                acc1, m21, img1 = got[1][path]
                acc0, m20, img0 = got[0].get(path, (acc1, np.zeros_like(m21), None))
                assert np.array_equal(acc0, want_acc) and np.array_equal(acc1, acc0), what
                assert not m20.any(), what
                assert np.array_equal(m21, want_m2), "%s: the plane differs at %d pixels" % (what, int((m21 != want_m2).sum()))
                if img0 is not None:
                    assert all(np.array_equal(a, b) for a, b in zip(img0, img1)), what


def test_what_the_option_leaves_alone(dr, hk, plane, synth, tmp_path):
    ctx = plane
    sc = _load(dr, _cube(tmp_path))
    ctx.upload(sc)
    st, bg = dr.pack_settings13(sc.settings(), 1), sc.settings().background
    W, H = 136, 96
    # moments = 0: no plane, the accessors give zeros / NULL, the asynchronous call works as before
    ctx.set_option("moments", 0)
    assert ctx.get_option("moments") == 0 and ctx.get_option("denoise_variance") == 0
    ctx.accum_reset(W, H)
    assert _moments_ptr(dr, ctx) == (None, 0) and not ctx.accum_moments().any()
    ctx.render_accumulate_async(st, W, H, bg, 5, STRIDE, 3)
    ctx.synchronize()
    acc_async = ctx.accum_read()
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, 5, STRIDE, 3)
    assert np.array_equal(ctx.accum_read(), acc_async) and not ctx.accum_moments().any()
    with pytest.raises(dr.DogerayError, match="no moments plane"):
        ctx.error(st, W, H, 3, 1.0)
    # the option is read by dr_accum_reset: setting it alone makes no plane, a reset with 1 does, a reset with 0 drops it
    ctx.set_option("moments", 1)
    assert _moments_ptr(dr, ctx) == (None, 0)
    ctx.accum_reset(W, H)
    ptr, nbytes = _moments_ptr(dr, ctx)
    assert ptr and nbytes == W * H * 8 and not ctx.accum_moments().any()
    ctx.render_accumulate(st, W, H, bg, 5, STRIDE, 3)
    assert np.array_equal(ctx.accum_read(), acc_async) and ctx.accum_moments().any()
    ctx.accum_reset(W, H)
    assert _moments_ptr(dr, ctx) == (ptr, nbytes) and not ctx.accum_moments().any()      # the allocation is kept, the plane is zeroed
    ctx.render_accumulate(st, W, H, bg, 5, STRIDE, 3)
    # dr_accum_error changes neither the accumulator, nor the plane, dr_stats or any option
    opts = {k: ctx.get_option(k) for k in ("kernel", "traversal", "pipe_group", "batch_frames", "denoise_tiles", "camera_cert", "moments", "denoise_variance")}
    acc, m2, before = ctx.accum_read(), ctx.accum_moments(), ctx.stats()
    ctx.error(st, W, H, 3, 0.5, sigma=True)
    assert ctx.stats() == before and {k: ctx.get_option(k) for k in opts} == opts
    assert np.array_equal(ctx.accum_read(), acc) and np.array_equal(ctx.accum_moments(), m2)
    ctx.set_option("moments", 0)
    ctx.accum_reset(W, H)
    assert _moments_ptr(dr, ctx) == (None, 0) and not ctx.accum_moments().any()


def _check_error(hk, ctx, st, W, H, n, tol, what):
    acc, hist, m2 = ctx.accum_read(), ctx.accum_history(), ctx.accum_moments()
    got = ctx.error(st, W, H, n, tol, sigma=True)
    sig, res = hk.error(acc, hist if hist.any() else None, m2, st, n, tol, nthreads=8)
    plane_got = got.pop("sigma")
    assert got == res, "%s: %s, host build %s" % (what, got, res)
    assert dc.same_bits(plane_got, sig), "%s: sigma differs at %d pixels" % (what, int((dc.bits(plane_got) != dc.bits(sig)).sum()))
    assert ctx.error(st, W, H, n, tol) == res, what
    return sig, res


def test_error_equals_the_host_build(dr, hk, plane, synth, tmp_path):
    import torch
    ctx = plane
    for name, W, H in (("cube", 136, 96), ("matball", 120, 88)):
        path = _scene(synth, tmp_path, name)
        sc = _load(dr, path)
        ctx.upload(sc)
        st, bg = dr.pack_settings13(sc.settings(), 1), sc.settings().background
        st_b = rc.moves(st)["sideways"]
        ctx.accum_reset(W, H)
        done = 0
        for n in (0, 1, 2, 16):
            if n > done:
                ctx.render_accumulate_pipelined(st, W, H, bg, 9 + STRIDE * done, STRIDE, n - done)
                done = n
            for tol in (0.0, 1.0):
                sig, res = _check_error(hk, ctx, st, W, H, n, tol, "%s %d frames" % (name, n))
            assert res["estimated"] == (res["pixels"] if n >= 2 else 0)
        # the plane into a device buffer; the result is known when the call returns
        got = ctx.error(st, W, H, 16, 1.0, sigma=True, device=True)
        side = torch.zeros(1, device="cuda:0")
        side += got["sigma"].sum() * 0
        assert got["sigma"].is_cuda and dc.same_bits(got.pop("sigma").cpu().numpy(), sig) and got == res
        # after a reprojection: every pixel its own count, also with no new frame (divide_by 0)
        counts = ctx.reproject(st, st_b, W, H, 16, max_history=12)
        assert 0 < counts["valid"] < counts["pixels"]
        sig, res = _check_error(hk, ctx, st_b, W, H, 0, 1.0, name + " reprojected, no new frame")
        assert res["estimated"] == counts["valid"] and not sig.T[:W, :H][ctx.accum_history() == 0].any()
        ctx.render_accumulate(st_b, W, H, bg, 77, STRIDE, 2)
        sig, res = _check_error(hk, ctx, st_b, W, H, 2, 1.0, name + " reprojected, two frames")
        assert res["estimated"] == res["pixels"]
        half = st_b.copy()
        half[11] = 2
        sig, res = _check_error(hk, ctx, half, W, H, 2, 1.0, name + " half the grid")
        assert res["pixels"] < W * H // 3


def test_reprojected_plane_equals_the_host_build(dr, hk, plane, synth, tmp_path):
    ctx = plane
    for name, W, H in (("cube", 136, 96), ("matball", 120, 88)):
        path = _scene(synth, tmp_path, name)
        sc = _load(dr, path)
        ctx.upload(sc)
        st, bg = dr.pack_settings13(sc.settings(), 1), sc.settings().background
        scene = hk.Scene(path, "")
        ga = scene.aov(st, W, H)
        for move, st_b in rc.moves(st).items():
            gb = scene.aov(st_b, W, H)
            ctx.accum_reset(W, H)
            ctx.render_accumulate(st, W, H, bg, 3, STRIDE, 3)
            acc, m2 = ctx.accum_read(), ctx.accum_moments()
            counts = ctx.reproject(st, st_b, W, H, 3)
            want = hk.reproject(acc, None, 3, st, st_b, ga, gb, m2=m2)
            what = "%s %s" % (name, move)
            assert counts == want[2] and np.array_equal(ctx.accum_read(), want[0]) and np.array_equal(ctx.accum_history(), want[1]), what
            assert np.array_equal(ctx.accum_moments(), want[3]), what
            # and back with an incoming history plane, two frames later, beyond max_history: the plane is scaled like the sums
            ctx.render_accumulate(st_b, W, H, bg, 91, STRIDE, 2)
            acc1, hist1, m21 = ctx.accum_read(), ctx.accum_history(), ctx.accum_moments()
            counts = ctx.reproject(st_b, st, W, H, 2, max_history=4, normal_cos=0.95)
            want = hk.reproject(acc1, hist1, 2, st_b, st, gb, ga, m2=m21, max_history=4, normal_cos=0.95)
            assert counts == want[2] and np.array_equal(ctx.accum_read(), want[0]) and np.array_equal(ctx.accum_history(), want[1]), what + ", and back"
            assert np.array_equal(ctx.accum_moments(), want[3]), what + ", and back"
            if move == "sideways":
                assert (want[1] == 4).any() and not np.array_equal(want[3], m21)
    # a grid smaller than the accumulator: zeros outside it
    h1, h2 = st.copy(), rc.moves(st)["sideways"].copy()
    h1[11] = h2[11] = 2
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, 3, STRIDE, 2)
    ctx.reproject(h1, h2, W, H, 2)
    m2 = ctx.accum_moments()
    gw, gh = dc.grid(h1, W, H)
    assert m2[:gw, :gh].any() and not m2[gw:].any() and not m2[:, gh:].any()


@pytest.mark.parametrize("name", ["matball", "cube"])
def test_calibration(dr, hk, plane, synth, tmp_path, name):
    """256x256, 16 frames: the mean of the estimated variances over the measured mean squared error of the 16-frame mean luma against a
    4096-frame mean.  The estimator is unbiased, so the expected ratio is 1 / (1 + 16 / 4096) -- the reference's own variance is on the
    measured side; a missing / n, an n for an n - 1 or a wrong scale (256) would put it outside [0.5, 2]."""
    ctx = plane
    sc = _load(dr, _scene(synth, tmp_path, name))
    ctx.upload(sc)
    st, bg = dr.pack_settings13(sc.settings(), 1), sc.settings().background
    W, H, n = 256, 256, 16
    ctx.set_option("moments", 0)
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, 1000, STRIDE, 4096)
    ref = mc.luma(ctx.accum_read()).astype(np.float64) / 256 / 4096
    ctx.set_option("moments", 1)
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, 77, STRIDE, n)
    acc, m2 = ctx.accum_read(), ctx.accum_moments()
    res = ctx.error(st, W, H, n, 1.0)
    assert res["estimated"] == res["pixels"] == W * H
    estimate = res["sum_var_q16"] / 65536 / res["estimated"]
    measured = float(((mc.luma(acc).astype(np.float64) / 256 / n - ref) ** 2).mean())
    host = hk.error(acc, None, m2, st, n, 1.0, nthreads=8)[1]
    ratio = estimate / measured
    print("moments calibration %s: estimated variance %.4f, measured MSE %.4f, ratio %.4f (host build %.4f)" %
          (name, estimate, measured, ratio, host["sum_var_q16"] / 65536 / host["estimated"] / measured))
    assert host == res
    assert 0.5 <= ratio <= 2.0, ratio


def test_convergence(dr, plane, synth, tmp_path):
    ctx = plane
    sc = _load(dr, _cube(tmp_path))
    ctx.upload(sc)
    st, bg = dr.pack_settings13(sc.settings(), 1), sc.settings().background
    W, H = 256, 256
    tol = 2.0
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, 5, STRIDE, 4)
    at4 = ctx.error(st, W, H, 4, tol)
    ctx.render_accumulate(st, W, H, bg, 5 + 4 * STRIDE, STRIDE, 60)
    at64 = ctx.error(st, W, H, 64, tol)
    print("moments convergence: above %.1f at 4 frames %d, at 64 frames %d of %d" % (tol, at4["above"], at64["above"], at64["pixels"]))
    assert at64["above"] < at4["above"]
    # render_until is the loop written by hand
    permille = max(1, at64["above"] * 1000 // at64["pixels"] + 40)         # reached somewhere between 4 and 64 frames
    ctx.accum_reset(W, H)
    frames, result = ctx.render_until(st, W, H, bg, 5, STRIDE, tol, permille, 96, check_every=8)
    acc_until = ctx.accum_read()
    ctx.accum_reset(W, H)
    n, hand = 0, None
    while n < 96:
        ctx.render_accumulate_pipelined(st, W, H, bg, 5 + n * STRIDE, STRIDE, 8)
        n += 8
        hand = ctx.error(st, W, H, n, tol)
        if hand["above"] + (hand["pixels"] - hand["estimated"]) <= permille * hand["pixels"] / 1000:
            break
    print("moments render_until: %d frames, %s" % (frames, result))
    assert (frames, result) == (n, hand) and np.array_equal(ctx.accum_read(), acc_until)
    assert 8 <= frames <= 96 and frames % 8 == 0, frames
    # a tolerance of 0 stops at max_frames, a huge one after the first chunk
    ctx.accum_reset(W, H)
    frames, result = ctx.render_until(st, W, H, bg, 5, STRIDE, 0.0, 0, 20, check_every=8)
    assert frames == 20 and result["above"] > 0
    ctx.accum_reset(W, H)
    frames, result = ctx.render_until(st, W, H, bg, 5, STRIDE, 1e9, 0, 96, check_every=8)
    assert frames == 8 and result["above"] == 0 and result["estimated"] == result["pixels"]


@pytest.mark.parametrize("name", ["matball", "cube"])
def test_denoiser_with_the_temporal_variance(dr, hk, plane, synth, tmp_path, name):
    """option denoise_variance = 1: bit for bit the host build with the same planes; at 4 and 16 frames (256x256) the denoised image's MSE
    against a 4096-frame mean is at most half the raw mean's, the bar of test_gpu_denoise.py.  Both variants' MSE are printed."""
    ctx = plane
    path = _scene(synth, tmp_path, name)
    sc = _load(dr, path)
    ctx.upload(sc)
    st, bg = dr.pack_settings13(sc.settings(), 1), sc.settings().background
    W, H = 256, 256
    ctx.set_option("moments", 0)
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, 1000, STRIDE, 4096)
    ref = ctx.accum_read().astype(np.float64).transpose(1, 0, 2) / 4096
    ctx.set_option("moments", 1)
    a = hk.Scene(path, "").aov(st, W, H)
    g = (a["normal"], a["albedo"], a["depth"], a["material"])
    ctx.accum_reset(W, H)
    done = 0
    for n in (4, 16):
        ctx.render_accumulate(st, W, H, bg, 77 + done * STRIDE, STRIDE, n - done)
        done = n
        acc, m2 = ctx.accum_read(), ctx.accum_moments()
        raw = acc.astype(np.float64).transpose(1, 0, 2) / n
        ctx.set_option("denoise_variance", 0)
        rgb0, f0 = ctx.denoise(st, W, H, n, out="both")
        want = hk.denoise(acc, st, n, *g, nthreads=8)
        assert dc.same_bits(f0, want[0]) and np.array_equal(rgb0, want[1]), (name, n)
        ctx.set_option("denoise_variance", 1)
        rgb1, f1 = ctx.denoise(st, W, H, n, out="both")
        want = hk.denoise(acc, st, n, *g, nthreads=8, m2=m2)
        assert dc.same_bits(f1, want[0]) and np.array_equal(rgb1, want[1]), (name, n)
        assert not dc.same_bits(f0, f1)
        mse = [float(((x.astype(np.float64) - ref) ** 2).mean()) for x in (raw, f0, f1)]
        print("moments denoise %s %d frames: MSE raw %.3f, spatial variance %.3f (ratio %.3f), temporal variance %.3f (ratio %.3f)" %
              (name, n, mse[0], mse[1], mse[1] / mse[0], mse[2], mse[2] / mse[0]))
        assert mse[2] <= 0.5 * mse[0], (n, mse)
    # without a plane the option changes nothing
    ctx.set_option("moments", 0)
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, 77, STRIDE, 4)
    on = ctx.denoise(st, W, H, 4, out="f32")
    ctx.set_option("denoise_variance", 0)
    assert dc.same_bits(on, ctx.denoise(st, W, H, 4, out="f32"))


def test_errors(dr, plane, synth, tmp_path):
    ctx = plane
    sc = _load(dr, _cube(tmp_path))
    st, bg = dr.pack_settings13(sc.settings(), 1), sc.settings().background
    W, H = 136, 96
    empty = dr.Context(0)
    try:
        with pytest.raises(dr.DogerayError, match="no scene") as e:
            empty.error(st, W, H, 1, 1.0)
        assert e.value.code == dr.ERR_INVALID
        empty.upload(sc)
        with pytest.raises(dr.DogerayError, match="accumulator") as e:
            empty.error(st, W, H, 1, 1.0)
        assert e.value.code == dr.ERR_INVALID
        empty.accum_reset(W, H)
        with pytest.raises(dr.DogerayError, match="no moments plane") as e:
            empty.error(st, W, H, 1, 1.0)
        assert e.value.code == dr.ERR_INVALID
        for bad in (2, -1):
            with pytest.raises(dr.DogerayError, match="not supported"):
                empty.set_option("moments", bad)
            with pytest.raises(dr.DogerayError, match="not supported"):
                empty.set_option("denoise_variance", bad)
    finally:
        empty.close()
    ctx.upload(sc)
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, 3, STRIDE, 2)
    acc, m2 = ctx.accum_read(), ctx.accum_moments()
    bad = st.copy()
    bad[11] = 0
    for args, msg in (((st, 128, H, 2, 1.0), "accumulator"), ((st, W, 95, 2, 1.0), "accumulator"), ((st, W, H, -1, 1.0), "divide_by"),
                      ((st, W, H, 2, -0.5), "tolerance"), ((st, W, H, 2, float("nan")), "tolerance"), ((bad, W, H, 2, 1.0), "divisor")):
        with pytest.raises(dr.DogerayError, match=msg) as e:
            ctx.error(*args)
        assert e.value.code == dr.ERR_INVALID, args[1:]
    rc_ = dr.lib().dr_accum_error(ctx._h, st.ctypes.data_as(C.c_void_p), W, H, 2, C.c_float(1.0), None, None, 0)
    assert rc_ == dr.ERR_INVALID and b"no output" in dr.lib().dr_last_error()
    with pytest.raises(dr.DogerayError, match="moments") as e:
        ctx.render_accumulate_async(st, W, H, bg, 3, STRIDE, 2)
    assert e.value.code == dr.ERR_INVALID
    ctx.synchronize()
    # none of the refused calls touched the accumulator or the plane
    assert np.array_equal(ctx.accum_read(), acc) and np.array_equal(ctx.accum_moments(), m2) and m2.any()


def test_full_size_c4(dr, hk):
    """The 1M-triangle C4 stand-in at 1920x1080, four pipelined frames: plane and error result equal the host build"""
    sys.path.insert(0, ROOT)
    import bench
    path = bench.ensure_scene(os.environ.get("DOGERAY_BENCH_CACHE", "/tmp/dogeray_bench"), 709, 1920, 1080)
    sc = dr.Scene.load(path, "")
    sc.build_bvh()
    W, H = 1920, 1080
    c = dr.Context(0)
    try:
        c.upload(sc)
        st, bg = dr.pack_settings13(sc.settings(), 1), sc.settings().background
        c.set_option("moments", 1)
        c.accum_reset(W, H)
        c.render_accumulate_pipelined(st, W, H, bg, 3, STRIDE, 4)
        acc, m2 = c.accum_read(), c.accum_moments()
        got = c.error(st, W, H, 4, 1.0, sigma=True)
        want_acc, want_m2 = _host_planes(hk, c, st, W, H, bg, [3 + STRIDE * k for k in range(4)])
    finally:
        c.close()
    assert np.array_equal(acc, want_acc) and np.array_equal(m2, want_m2)
    sig, res = hk.error(acc, None, m2, st, 4, 1.0, nthreads=8)
    plane_got = got.pop("sigma")
    print("moments C4 1920x1080, 4 frames: %s" % got)
    assert got == res and dc.same_bits(plane_got, sig)


def test_cli_until_sigma(dr, plane, tmp_path):
    ctx = plane
    path = _cube(tmp_path)
    exe = os.path.join(ROOT, "dogeray_amd", "bin", "dogeray")
    sigma_out = str(tmp_path / "sigma.pfm")
    sc = _load(dr, path)
    ctx.upload(sc)
    W, H = sc.settings().width, sc.settings().height
    for tol, permille, max_frames in ((4.0, 200, 64), (0.0, 0, 16)):
        r = subprocess.run(["timeout", "-k", "10", "120", exe, path, "--quiet", "--until-sigma", "%r,%d" % (tol, permille), "--max-frames", str(max_frames),
                            "--sigma-out", sigma_out], capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        m = re.search(r"^(converged|not converged) after (\d+) frames: (\d+) of (\d+) pixels above (\S+)$", r.stdout, re.M)
        assert m, r.stdout
        pr = dr.ProgressiveRenderer(ctx, sc.settings())
        for _ in range(4):
            td, div = pr.step()
        assert div == 1
        frames, result = pr.run_until(tol, permille, max_frames)
        print("moments CLI: %s; run_until %d frames, %s" % (m.group(0), frames, result))
        assert (int(m.group(2)), int(m.group(3)), int(m.group(4))) == (frames, result["above"], result["pixels"])
        assert (m.group(1) == "converged") == dr.Context.converged(result, permille) and float(m.group(5)) == tol
        assert (m.group(1) == "converged") == (tol > 0)
        assert pr.iter - pr._pnum == 1 + frames
        sigma = ctx.error(pr.settings13(), W, H, 1 + frames, 0.0, sigma=True)["sigma"]
        assert "exported noise estimate:" in r.stdout
        assert dc.same_bits(dr.read_pfm(sigma_out), sigma) and sigma.any()
    # --sigma-out alone: the fixed frame count, with a plane
    r = subprocess.run(["timeout", "-k", "10", "120", exe, path, "--quiet", "--frames", "3", "--sigma-out", sigma_out], capture_output=True, text=True,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    pr = dr.ProgressiveRenderer(ctx, sc.settings())
    for _ in range(7):
        td, div = pr.step()
    assert dc.same_bits(dr.read_pfm(sigma_out), ctx.error(pr.settings13(), W, H, div, 0.0, sigma=True)["sigma"])
