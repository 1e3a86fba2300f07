"""The temporal reprojection on the GPU (dr_accum_reproject / Context.reproject, ProgressiveRenderer.move_camera, dogeray --move-to): bit for bit
the host build of the same device functions (tools/host_kernel.cpp hk_reproject) on the same accumulator and guides, the consumers of the history
plane (present, denoiser, pipelined presents), the guide cache, ordering behind the pipeline, what it leaves alone, image quality after a camera
move against a long mean, and its errors."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import CUBE_SETTINGS, ROOT, SCENES, with_settings
import denoise_checks as dc
import reproject_checks as rc

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))
GUIDES = ("t", "normal", "material")


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


def _cases(synth, tmp_path):
    cube = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube.rts"), CUBE_SETTINGS)
    textest = os.path.join(SCENES, "textest.rts")
    if not any(l.startswith("*") for l in open(textest)):
        textest = with_settings(textest, str(tmp_path / "textest.rts"), CUBE_SETTINGS)
    return (("cube", cube, 136, 96), ("matball", os.path.join(synth["dir"], "matball.rts"), 120, 88), ("textest", textest, 136, 96),
            ("hf_small", os.path.join(synth["dir"], "hf_small.rts"), 160, 96))


def _cube256(tmp_path):
    return with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube256.rts"), CUBE_SETTINGS)


def _load(dr, path):
    sc = dr.Scene.load(path, "")
    sc.build_bvh()
    return sc


def _render(ctx, sc, st, W, H, frames, seed=3):
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, sc.settings().background, seed, 1000003, frames)
    return ctx.accum_read()


def _same(ctx, counts, want, what):
    acc, hist = ctx.accum_read(), ctx.accum_history()
    assert counts == want[2], "%s: counts %s, host build %s" % (what, counts, want[2])
    assert sum(counts[k] for k in rc.CLASSES) == counts["pixels"], what
    assert np.array_equal(acc, want[0]), "%s: sums differ at %d values" % (what, int((acc != want[0]).sum()))
    assert np.array_equal(hist, want[1]), "%s: history differs at %d pixels" % (what, int((hist != want[1]).sum()))
    return acc, hist


def _trunc_div(a, d):
    """integer division towards zero, 0 where the divisor is 0"""
    a, d = a.astype(np.int64), np.broadcast_to(d.astype(np.int64), a.shape)
    safe = np.where(d == 0, 1, d)
    return np.where(d == 0, 0, np.sign(a) * np.sign(safe) * (np.abs(a) // np.abs(safe)))


def _present(acc, hist, div):
    return np.clip(_trunc_div(acc, (hist + div)[..., None]), 0, 255).astype(np.uint8).transpose(1, 0, 2)


@pytest.mark.parametrize("mode", [2, 0, 1])
def test_gpu_equals_the_host_build(dr, hk, ctx, synth, tmp_path, mode):
    for name, path, W, H in _cases(synth, tmp_path):
        sc = _load(dr, path)
        ctx.upload(sc)
        ctx.set_traversal(mode)
        st = dr.pack_settings13(sc.settings(), 1)
        scene = hk.Scene(path, "")
        ga = scene.aov(st, W, H)
        first = True
        for move, st_b in rc.moves(st).items():
            gb = scene.aov(st_b, W, H)
            acc = _render(ctx, sc, st, W, H, 3)
            assert not ctx.accum_history().any()
            counts = ctx.reproject(st, st_b, W, H, 3)
            what = "%s %s traversal %d" % (name, move, mode)
            _same(ctx, counts, hk.reproject(acc, None, 3, st, st_b, ga, gb), what)
            if first:                          # the restatement, once per scene
                ca, cb = hk.camera_block(st, W, H), hk.camera_block(st_b, W, H)
                _same(ctx, counts, rc.reproject(acc, None, 3, ca, cb, ga, gb, ca["gw"], ca["gh"]), what + ": restatement")
                first = False
            if mode == 2:                      # and back with an incoming history plane, two frames later, beyond max_history
                ctx.render_accumulate(st_b, W, H, sc.settings().background, 91, 1000003, 2)
                acc1, hist1 = ctx.accum_read(), ctx.accum_history()
                counts = ctx.reproject(st_b, st, W, H, 2, max_history=4, normal_cos=0.95)
                _same(ctx, counts, hk.reproject(acc1, hist1, 2, st_b, st, gb, ga, max_history=4, normal_cos=0.95), what + ", and back")
    ctx.set_traversal(2)


def test_consumers_of_the_history_plane(dr, hk, ctx, synth, tmp_path):
    path = _cube256(tmp_path)
    sc = _load(dr, path)
    ctx.set_traversal(2)
    ctx.upload(sc)
    s = sc.settings()
    st = dr.pack_settings13(s, 1)
    st_b = rc.moves(st)["sideways"]
    W, H = 256, 256
    _render(ctx, sc, st, W, H, 4)
    counts = ctx.reproject(st, st_b, W, H, 4)
    assert counts["valid"] > 0 and counts["valid"] < counts["pixels"]
    ctx.render_accumulate(st_b, W, H, s.background, 55, 1000003, 1)
    acc, hist = ctx.accum_read(), ctx.accum_history()
    assert set(np.unique(hist)) == {0, 4}
    ptr, nbytes = C.c_void_p(), C.c_uint64()
    assert dr.lib().dr_accum_history_device_ptr(ctx._h, C.byref(ptr), C.byref(nbytes)) == 0 and ptr.value and nbytes.value == W * H * 4
    # present and denoiser divide every pixel by its own count
    assert np.array_equal(ctx.accum_present(1), _present(acc, hist, 1))
    gb = hk.Scene(path, "").aov(st_b, W, H)
    for params in ({}, {"iterations": 0}, {"iterations": 2, "demodulate": 0}):
        rgb, f = ctx.denoise(st_b, W, H, 1, out="both", **params)
        wf, wr = hk.denoise(acc, st_b, 1, gb["normal"], gb["albedo"], gb["depth"], gb["material"], hist=hist, **params)
        assert dc.same_bits(f, wf) and np.array_equal(rgb, wr), params
    assert np.array_equal(ctx.denoise(st_b, W, H, 1, iterations=0), ctx.accum_present(1))
    # the presents of three pipelined frames
    seeds = [101 + 1000003 * k for k in range(3)]
    tickets = [ctx.pipeline_submit(st_b, W, H, s.background, seeds[k], present_divide_by=k + 2) for k in range(3)]
    images = [ctx.pipeline_wait(t, want_image=True) for t in tickets]
    total = acc.astype(np.int64)
    for k in range(3):
        total = total + ctx.render_frame(st_b, W, H, s.background, seeds[k])
        assert np.array_equal(images[k], _present(total, hist, k + 2)), "pipelined present %d" % k
    assert np.array_equal(ctx.accum_read(), total) and np.array_equal(ctx.accum_history(), hist)
    # dr_accum_reset drops the plane: present and denoise are what they are on a context that never reprojected
    got = _render(ctx, sc, st_b, W, H, 2, seed=8)
    assert not ctx.accum_history().any()
    assert dr.lib().dr_accum_history_device_ptr(ctx._h, C.byref(ptr), C.byref(nbytes)) == 0 and not ptr.value and nbytes.value == 0
    fresh = dr.Context(0)
    try:
        fresh.upload(sc)
        assert np.array_equal(_render(fresh, sc, st_b, W, H, 2, seed=8), got)
        assert not fresh.accum_history().any()
        assert np.array_equal(fresh.accum_present(2), ctx.accum_present(2))
        a, b = fresh.denoise(st_b, W, H, 2, out="both"), ctx.denoise(st_b, W, H, 2, out="both")
        assert np.array_equal(a[0], b[0]) and dc.same_bits(a[1], b[1])
    finally:
        fresh.close()


def test_guide_cache_ordering_and_what_it_leaves_alone(dr, hk, ctx, synth, tmp_path):
    path = _cube256(tmp_path)
    sc = _load(dr, path)
    ctx.set_traversal(2)
    ctx.upload(sc)
    s = sc.settings()
    st_a = dr.pack_settings13(s, 1)
    mv = rc.moves(st_a)
    st_b, st_c = mv["sideways"], mv["dolly"]
    W, H = 256, 256
    scene = hk.Scene(path, "")
    ga, gb, gc = scene.aov(st_a, W, H), scene.aov(st_b, W, H), scene.aov(st_c, W, H)
    acc = _render(ctx, sc, st_a, W, H, 2)
    opts = {k: ctx.get_option(k) for k in ("kernel", "traversal", "pipe_group", "batch_frames", "denoise_tiles", "camera_cert")}
    before = ctx.stats()
    # A -> B traces both views, B -> C only C
    _same(ctx, ctx.reproject(st_a, st_b, W, H, 2), hk.reproject(acc, None, 2, st_a, st_b, ga, gb), "A -> B")
    assert ctx.get_option("reproject_aov_passes") == 2
    acc, hist = ctx.accum_read(), ctx.accum_history()
    _same(ctx, ctx.reproject(st_b, st_c, W, H, 1), hk.reproject(acc, hist, 1, st_b, st_c, gb, gc), "B -> C")
    assert ctx.get_option("reproject_aov_passes") == 1
    assert ctx.stats() == before and {k: ctx.get_option(k) for k in opts} == opts
    # a view that is not the cached one: two passes again; the same view twice: the cached planes serve both sides
    acc, hist = ctx.accum_read(), ctx.accum_history()
    _same(ctx, ctx.reproject(st_a, st_b, W, H, 1), hk.reproject(acc, hist, 1, st_a, st_b, ga, gb), "A -> B, not cached")
    assert ctx.get_option("reproject_aov_passes") == 2
    acc, hist = ctx.accum_read(), ctx.accum_history()
    _same(ctx, ctx.reproject(st_b, st_b, W, H, 1), hk.reproject(acc, hist, 1, st_b, st_b, gb, gb), "B -> B")
    assert ctx.get_option("reproject_aov_passes") == 0
    # a scene upload drops the cache
    ctx.upload(sc)
    acc, hist = ctx.accum_read(), ctx.accum_history()
    _same(ctx, ctx.reproject(st_b, st_c, W, H, 1), hk.reproject(acc, hist, 1, st_b, st_c, gb, gc), "B -> C after an upload")
    assert ctx.get_option("reproject_aov_passes") == 2
    # ordered behind dr_pipeline_submit: the call sees every frame submitted before it
    ctx.accum_reset(W, H)
    seeds = [11 + 1000003 * k for k in range(3)]
    tickets = [ctx.pipeline_submit(st_a, W, H, s.background, seeds[k]) for k in range(3)]
    counts = ctx.reproject(st_a, st_b, W, H, 3)
    for t in tickets:
        ctx.pipeline_wait(t)
    total = sum(ctx.render_frame(st_a, W, H, s.background, sd).astype(np.int64) for sd in seeds).astype(np.int32)
    _same(ctx, counts, hk.reproject(total, None, 3, st_a, st_b, ga, gb), "behind the pipeline")


@pytest.mark.parametrize("name", ["matball", "cube"])
def test_quality_after_a_camera_move(dr, ctx, synth, tmp_path, name):
    """256x256: 16 frames in view A, reprojected into view B (the camera 5 % of its distance to the look-at point further sideways), one more
    frame there.  Over the valid pixels the MSE against a 4096-frame mean of view B is at most half that of one frame rendered from scratch in
    B with the same seed -- carrying 16 samples predicts about 1/17 of the raw variance, the half leaves the rest for the nearest-neighbour
    resampling error (the denoiser's bar) -- and the valid pixels are at least half of the pixels of B whose material is carried at all."""
    path = os.path.join(synth["dir"], "matball.rts") if name == "matball" else with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "c.rts"), CUBE_SETTINGS)
    sc = _load(dr, path)
    ctx.set_traversal(2)
    ctx.upload(sc)
    st_a = dr.pack_settings13(sc.settings(), 1)
    st_b = rc.moves(st_a)["sideways"]
    W, H = 256, 256
    ref = _render(ctx, sc, st_b, W, H, 4096, seed=1000).astype(np.float64) / 4096
    raw = _render(ctx, sc, st_b, W, H, 1, seed=500).astype(np.float64)
    _render(ctx, sc, st_a, W, H, 16, seed=77)
    counts = ctx.reproject(st_a, st_b, W, H, 16)
    ctx.render_accumulate(st_b, W, H, sc.settings().background, 500, 1000003, 1)
    acc, hist = ctx.accum_read().astype(np.float64), ctx.accum_history()
    img = acc / (hist + 1)[..., None]
    valid = hist > 0
    carried = rc.allowed(ctx.render_aov(st_b, W, H, channels=("material",))["material"], rc.DEFAULTS).T
    assert int(valid.sum()) == counts["valid"] and (hist[valid] == 16).all()
    mse_raw, mse_rep = float(((raw - ref)[valid] ** 2).mean()), float(((img - ref)[valid] ** 2).mean())
    print("reproject quality %s: valid %d of %d carried-material pixels (%.3f), MSE one frame %.3f reprojected %.3f ratio %.3f" %
          (name, counts["valid"], int(carried.sum()), counts["valid"] / carried.sum(), mse_raw, mse_rep, mse_rep / mse_raw))
    assert 2 * counts["valid"] >= int(carried.sum()), counts
    assert mse_rep <= 0.5 * mse_raw, (mse_raw, mse_rep)


def test_full_size_c4(dr, hk):
    """The 1M-triangle C4 stand-in at 1920x1080: the GPU equals hk_reproject fed with the GPU's own AOVs"""
    sys.path.insert(0, ROOT)
    import bench
    path = bench.ensure_scene(os.environ.get("DOGERAY_BENCH_CACHE", "/tmp/dogeray_bench"), 709, 1920, 1080)
    sc = dr.Scene.load(path, "")
    sc.build_bvh()
    c = dr.Context(0)
    try:
        c.upload(sc)
        st = dr.pack_settings13(sc.settings(), 1)
        st_b = rc.moves(st)["sideways"]
        acc = _render(c, sc, st, 1920, 1080, 2)
        counts = c.reproject(st, st_b, 1920, 1080, 2)
        got_acc, got_hist = c.accum_read(), c.accum_history()
        ga, gb = c.render_aov(st, 1920, 1080, channels=GUIDES), c.render_aov(st_b, 1920, 1080, channels=GUIDES)
    finally:
        c.close()
    want = hk.reproject(acc, None, 2, st, st_b, ga, gb, nthreads=8)
    print("reproject C4 1920x1080: %s" % counts)
    assert counts == want[2] and np.array_equal(got_acc, want[0]) and np.array_equal(got_hist, want[1])


def test_cli_moves_the_camera(dr, ctx, tmp_path):
    path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube.rts"), CUBE_SETTINGS)
    exe = os.path.join(ROOT, "dogeray_amd", "bin", "dogeray")
    out, den = str(tmp_path / "moved.ppm"), str(tmp_path / "moved_den.ppm")
    target = (7.75, -6.5, 4.875, 0.25, 0.125, 0.0)                # exact in float32 and in the text
    r = subprocess.run(["timeout", "-k", "10", "120", exe, path, "--frames", "3", "--quiet", "--out", out, "--denoise", den, "--move-to",
                        ",".join(repr(v) for v in target), "--move-frames", "2"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    m = re.search(r"reprojected: (\d+) pixels, (\d+) valid, (\d+) masked, (\d+) offscreen, (\d+) rejected", r.stdout)
    assert m, r.stdout
    sc = _load(dr, path)
    ctx.set_traversal(2)
    ctx.upload(sc)
    pr = dr.ProgressiveRenderer(ctx, sc.settings())
    for _ in range(7):                        # the CLI's present loop: four preview steps and three frames
        td, div = pr.step()
    assert div == 4
    moved = type(sc.settings()).from_buffer_copy(sc.settings())
    moved.campos[:] = target[:3]
    moved.look[:] = target[3:]
    counts = pr.move_camera(moved)
    assert [int(v) for v in m.groups()] == [counts[k] for k in ("pixels",) + rc.CLASSES] and counts["valid"] > 0
    assert [pr.step()[1] for _ in range(2)] == [1, 2]
    assert np.array_equal(pr.settings13(), dr.pack_settings13(moved, 1))
    W, H = pr.W, pr.H
    data = open(out, "rb").read()
    assert data.startswith(b"P6\n%d %d\n255\n" % (W, H))
    img = pr.image(2)
    assert np.array_equal(np.frombuffer(data[-W * H * 3:], np.uint8).reshape(img.shape), img)
    assert np.array_equal(img, _present(ctx.accum_read(), ctx.accum_history(), 2)) and ctx.accum_history().any()
    data = open(den, "rb").read()
    assert np.array_equal(np.frombuffer(data[-W * H * 3:], np.uint8).reshape(img.shape), pr.image(2, denoise=True))
    # reproject=False: the reference's behaviour, the ladder starts again
    assert pr.move_camera(sc.settings(), reproject=False) is None and pr.iter == 0 and not ctx.accum_history().any()
    assert pr.step() == (8, 1)


def test_reproject_errors(dr, ctx, synth, tmp_path):
    st0 = np.zeros(13, np.float32) + 1
    path = _cube256(tmp_path)
    sc = _load(dr, path)
    st = dr.pack_settings13(sc.settings(), 1)
    st_b = rc.moves(st)["sideways"]
    empty = dr.Context(0)
    try:
        with pytest.raises(dr.DogerayError, match="no scene") as e:
            empty.reproject(st0, st0, 64, 64, 1)
        assert e.value.code == dr.ERR_INVALID
        empty.upload(sc)
        with pytest.raises(dr.DogerayError, match="accumulator") as e:
            empty.reproject(st, st_b, 256, 256, 1)
        assert e.value.code == dr.ERR_INVALID
        assert empty.get_option("reproject_aov_passes") == 0
    finally:
        empty.close()
    ctx.set_traversal(2)
    ctx.upload(sc)
    acc = _render(ctx, sc, st, 256, 256, 1)
    half, bad, flat = st_b.copy(), st_b.copy(), st.copy()
    half[11] = 2
    bad[11] = 0
    flat[7] = 0                                   # focus distance 0: the `from` view's focus plane collapses into the pinhole
    cases = [((st, st_b, 128, 256, 1), {}, "accumulator"), ((st, st_b, 256, 255, 1), {}, "accumulator"), ((st, st_b, 256, 256, 0), {}, "frames"),
             ((st, st_b, 256, 256, -2), {}, "frames"), ((st, half, 256, 256, 1), {}, "divisors"), ((half, st, 256, 256, 1), {}, "divisors"),
             ((st, bad, 256, 256, 1), {}, "divisor"), ((flat, st_b, 256, 256, 1), {}, "degenerate"),
             ((st, st_b, 256, 256, 1), {"max_history": 0}, "max_history"), ((st, st_b, 256, 256, 1), {"max_history": 65536}, "max_history"),
             ((st, st_b, 256, 256, 1), {"normal_cos": 1.25}, "normal_cos"), ((st, st_b, 256, 256, 1), {"plane_tolerance": -1.0}, "plane_tolerance")]
    for args, params, msg in cases:
        with pytest.raises(dr.DogerayError, match=msg) as e:
            ctx.reproject(*args, **params)
        assert e.value.code == dr.ERR_INVALID, (args[2:], params)
    ctx.set_stripe(2, 0)
    try:
        with pytest.raises(dr.DogerayError, match="stripe") as e:
            ctx.reproject(st, st_b, 256, 256, 1)
        assert e.value.code == dr.ERR_INVALID
    finally:
        ctx.set_stripe(1, 0)
    with pytest.raises(TypeError):
        ctx.reproject(st, st_b, 256, 256, 1, history=3)
    # none of the refused calls touched the accumulator or made a history plane
    assert np.array_equal(ctx.accum_read(), acc) and not ctx.accum_history().any()
    # a grid smaller than the accumulator: zeros outside it
    h2 = st.copy()
    h2[11] = 2
    counts = ctx.reproject(h2, half, 256, 256, 1)
    assert counts["pixels"] == 128 * 128
    a, h = ctx.accum_read(), ctx.accum_history()
    assert not a[128:].any() and not a[:, 128:].any() and not h[128:].any() and not h[:, 128:].any() and h[:128, :128].any()
