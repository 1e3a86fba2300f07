"""Adaptive sampling on the GPU (dr_render_adaptive / Context.render_adaptive, Context.adaptive_tiles, Context.render_until_adaptive,
ProgressiveRenderer.run_until_adaptive, dogeray --until-sigma --adaptive): a pass against its definition -- the flags of the host build of the same
device functions (tools/host_kernel.cpp) and of the numpy restatement (tests/adaptive_checks.py), the planes against the GPU's own frames
(Context.render_frame) folded by the host build under the mask, bit for bit --, through both group sizes and traversals, before and after the
tile order exists, with eight queues and an empty one, over the adversarial planes of tests/plane_cases.py, behind a reprojection; what a pass
leaves alone; the loop; the refusals."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import CUBE_SETTINGS, ROOT, SCENES, with_settings
import adaptive_checks as ac
import device_planes as dp
import plane_cases as pc
import reproject_checks as rc

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))
STRIDE = 1000003
BASE_SEED, PASS_SEED = 31, 31 + 4 * STRIDE


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
def shared(dr, synth):          # synth first: the generated scenes exist before this process touches the GPU
    c = dr.Context(0)
    yield c
    c.close()


OPTIONS = ("moments", "pipe_group", "feedback", "short_one_queue", "sky_tiles", "kernel")


@pytest.fixture()
def ctx(shared):
    """the shared context with a second-moment plane for the test, and as it was afterwards"""
    before = {k: shared.get_option(k) for k in OPTIONS}
    shared.set_traversal(2)
    shared.set_option("moments", 1)
    yield shared
    for k, v in before.items():
        shared.set_option(k, v)
    shared.set_traversal(2)


def _cube(tmp_path):
    return with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube.rts"), CUBE_SETTINGS)


def _scene(synth, tmp_path, name):
    return os.path.join(synth["dir"], "matball.rts") if name == "matball" else _cube(tmp_path)


def _load(dr, path):
    sc = dr.Scene.load(path, "")
    sc.build_bvh()
    return sc


def _median_tolerance(acc, hist, m2, gx, gy, divide_by):
    """the median over tiles of the tile-maximum sigma: about half of the tiles hold a pixel above it"""
    return float(np.median(ac.tile_max_sigma(acc, hist, m2, gx, gy, divide_by)))


def check_pass(dr, hk, ctx, st, W, H, bg, seed, nframes, divide_by, base, **params):
    """One pass from the planes `base` = (acc, hist, m2) as read back (hist all zeros where there is no plane yet): the result, the flags and the
    three planes against the definition.  Returns (result, flags)."""
    acc, hist, m2 = base
    gx, gy = ac.grid(st, W, H)
    r = ctx.render_adaptive(st, W, H, bg, seed, STRIDE, nframes, divide_by, **params)
    flags = ctx.adaptive_tiles()
    got = dp.peek(ctx)
    want_flags, counts = hk.adaptive_select(acc, hist, m2, st, divide_by, **params)
    again, want = ac.select(acc, hist, m2, gx, gy, divide_by, **params)
    assert np.array_equal(flags, want_flags) and np.array_equal(flags, again)
    assert r == dict(want, samples_added=want["active_tiles"] * 64 * nframes), (r, want)
    frames = np.stack([ctx.render_frame(st, W, H, bg, seed + k * STRIDE) for k in range(nframes)])
    wa, wh, wm = hk.adaptive_add(acc.copy(), hist.copy(), m2.copy(), st, frames, np.nonzero(flags)[0].astype(np.int32))
    for name, g, w in (("sums", got[0], wa), ("history", got[1], wh), ("M2", got[2], wm)):
        assert np.array_equal(g, w), "%s differ at %d values" % (name, int((g != w).sum()))
    ra, rh, rm = ac.fold(acc, hist, m2, frames, flags, gx, gy)
    assert np.array_equal(wa, ra) and np.array_equal(wh, rh) and np.array_equal(wm, rm)
    m = ac.pixel_mask(flags, gx, gy, W, H)      # outside the active tiles, and outside the grid: the bits as they were
    assert np.array_equal(got[0][~m], acc[~m]) and np.array_equal(got[1][~m], hist[~m]) and np.array_equal(got[2][~m], m2[~m])
    return r, flags


# name, W, H: the cube at 136 x 96, the matball with a grid smaller than the accumulator (112 x 88 of 117 x 89), the cube in a single tile
VIEWS = (("cube", 136, 96), ("matball", 117, 89), ("cube", 13, 9))


@pytest.mark.parametrize("traversal", [2, 0])
@pytest.mark.parametrize("group", [1, 8])
def test_pass_equals_its_definition(dr, hk, ctx, synth, tmp_path, group, traversal):
    ctx.set_option("pipe_group", group)
    for name, W, H in VIEWS:
        sc = _load(dr, _scene(synth, tmp_path, name))
        ctx.upload(sc)
        ctx.set_traversal(traversal)
        st, bg = dr.pack_settings13(sc.settings(), 1), sc.settings().background
        gx, gy = ac.grid(st, W, H)
        for later in (False, True):      # the first launches of the view on this upload (no tile order yet), and launches after several
            ctx.accum_reset(W, H)
            ctx.render_accumulate(st, W, H, bg, BASE_SEED, STRIDE, 4)
            if later:
                for k in range(3):
                    ctx.render_frame(st, W, H, bg, 900 + k)
            base = dp.peek(ctx)
            assert not base[1].any() and base[2].any()
            if gx * gy == 1:
                for tol, active in ((0.0, 1), (1e9, 0)):
                    r, _ = check_pass(dr, hk, ctx, st, W, H, bg, PASS_SEED, 3, 4, base, tolerance=tol)
                    assert r["active_tiles"] == active and r["tiles"] == 1
                    base = dp.peek(ctx)
                continue
            tol = _median_tolerance(*base, gx, gy, 4)
            r, flags = check_pass(dr, hk, ctx, st, W, H, bg, PASS_SEED, 3, 4, base, tolerance=tol)
            assert 0 < r["active_tiles"] < r["tiles"] == gx * gy, (name, r)
            # a second pass on what the first left: per-pixel counts now differ between the tiles
            base = dp.peek(ctx)
            assert set(np.unique(base[1])) == {0, 3}
            check_pass(dr, hk, ctx, st, W, H, bg, PASS_SEED + 3 * STRIDE, 2, 4, base, tolerance=tol, tile_pixels=2, max_samples=7)


def test_feedback_off(dr, hk, ctx, tmp_path):
    sc = _load(dr, _cube(tmp_path))
    ctx.upload(sc)
    ctx.set_option("feedback", 0)
    st, bg, W, H = dr.pack_settings13(sc.settings(), 1), sc.settings().background, 136, 96
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, BASE_SEED, STRIDE, 4)
    base = dp.peek(ctx)
    r, _ = check_pass(dr, hk, ctx, st, W, H, bg, PASS_SEED, 3, 4, base, tolerance=_median_tolerance(*base, 17, 12, 4))
    assert 0 < r["active_tiles"] < r["tiles"]


def test_eight_queues_and_an_empty_one(dr, hk, ctx, tmp_path):
    """256 x 256: 1024 tiles in eight queues (short_one_queue 0: the plan keeps one queue per XCD); the cube's sky leaves a whole queue without an
    active tile"""
    sc = _load(dr, _cube(tmp_path))
    ctx.upload(sc)
    ctx.set_option("short_one_queue", 0)
    st, bg, W, H = dr.pack_settings13(sc.settings(), 1), sc.settings().background, 256, 256
    gx, gy = ac.grid(st, W, H)
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, BASE_SEED, STRIDE, 4)
    base = dp.peek(ctx)
    # the upper quarter of the tiles by their noisiest pixel: the cube, not its sky
    tol = float(np.quantile(ac.tile_max_sigma(*base, gx, gy, 4), 0.75))
    bands = [np.arange((1024 * q + 7) // 8, (1024 * (q + 1) + 7) // 8) for q in range(8)]      # make_params' queues of the identity order
    for order_exists in (True, False):
        if not order_exists:
            ctx.set_option("feedback", 0)      # drops the order: the identity
            assert ctx.tile_order() is None
            base = dp.peek(ctx)
        stored = ctx.tile_order()
        r, flags = check_pass(dr, hk, ctx, st, W, H, bg, PASS_SEED, 3, 4, base, tolerance=tol)
        assert 0 < r["active_tiles"] < r["tiles"] == 1024
        queues = [bands]
        if order_exists:
            assert stored is not None and stored["regions"] == 8 and stored["ntiles"] == 1024, "the view's launches do not use eight queues"
            queues.append([stored["order"][stored["region_start"][q]:stored["region_start"][q + 1]] for q in range(8)])
        for qs in queues:      # (whichever of the two the pass's launch used)
            per_queue = [int(flags[t].sum()) for t in qs]
            print("adaptive, eight queues: active tiles per queue %s" % per_queue)
            assert 0 in per_queue and max(per_queue) > 0, "no queue without an active tile: the case does not test what it is for"


def test_all_and_none(dr, ctx, synth, tmp_path):
    for name, W, H in (("cube", 136, 96), ("matball", 117, 89)):
        sc = _load(dr, _scene(synth, tmp_path, name))
        ctx.upload(sc)
        st, bg = dr.pack_settings13(sc.settings(), 1), sc.settings().background
        gx, gy = ac.grid(st, W, H)
        # everything asks (n = 0 < min_samples): the pass is render_accumulate_pipelined of the same seeds, with the count in the history plane
        ctx.accum_reset(W, H)
        ctx.render_accumulate_pipelined(st, W, H, bg, BASE_SEED, STRIDE, 5)
        want = dp.peek(ctx)
        ctx.accum_reset(W, H)
        r = ctx.render_adaptive(st, W, H, bg, BASE_SEED, STRIDE, 5, 0, tolerance=0.0, max_samples=0)
        got = dp.peek(ctx)
        assert r["active_tiles"] == r["tiles"] == gx * gy and r["asking_pixels"] == r["pixels"] and r["samples_added"] == gx * gy * 64 * 5
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
        assert np.array_equal(got[1], np.where(ac.pixel_mask(np.ones(gx * gy), gx, gy, W, H), 5, 0)) and ctx.adaptive_tiles().all()
        # nothing asks: n = 5 >= min_samples and no estimate is above 1e9
        r = ctx.render_adaptive(st, W, H, bg, PASS_SEED, STRIDE, 3, 0, tolerance=1e9)
        after = dp.peek(ctx)
        assert r["active_tiles"] == 0 and r["asking_pixels"] == 0 and r["samples_added"] == 0 and not ctx.adaptive_tiles().any()
        assert all(np.array_equal(a, b) for a, b in zip(after, got))


@pytest.mark.parametrize("size", [pc.BIG, pc.TAIL2, pc.TILE], ids=lambda s: "%dx%d" % s)
def test_adversarial_planes(dr, hk, ctx, tmp_path, size):
    W, H = size
    sc = _load(dr, _cube(tmp_path))
    ctx.upload(sc)
    st, bg = dr.pack_settings13(sc.settings(), 1), sc.settings().background
    gx, gy = ac.grid(st, W, H)
    ctx.accum_reset(W, H)
    dp.history(ctx, st, W, H)
    for name in ("wide", "mixed"):
        acc = pc.make_acc(name, W, H)
        base = dp.install(dr, ctx, acc=acc, hist=pc.hist(W, H), m2=pc.m2_wide(W, H, acc))
        est, sig = ac.sigma(*base, gx, gy, 3)
        tol = float(np.median(sig[est & np.isfinite(sig)]))
        results = []
        for divide_by, params in ((3, {"tolerance": tol, "tile_pixels": 33}), (0, {"tolerance": tol, "max_samples": 30000, "tile_pixels": 20})):
            results.append(check_pass(dr, hk, ctx, st, W, H, bg, PASS_SEED, 2, divide_by, base, **params)[0])
            base = dp.peek(ctx)
        if size == pc.BIG:
            assert 0 < results[0]["active_tiles"] < results[0]["tiles"], (name, results)


def test_with_a_reprojection(dr, hk, ctx, tmp_path):
    path = _cube(tmp_path)
    sc = _load(dr, path)
    ctx.upload(sc)
    st, bg, W, H = dr.pack_settings13(sc.settings(), 1), sc.settings().background, 136, 96
    st_b = rc.moves(st)["sideways"]
    gx, gy = ac.grid(st, W, H)
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, BASE_SEED, STRIDE, 16)
    ctx.reproject(st, st_b, W, H, 16)
    base = dp.peek(ctx)
    assert (base[1][:8 * gx, :8 * gy] == 0).any() and (base[1] == 16).any()      # disoccluded pixels at n = 0 beside neighbours with 16 samples
    tol = _median_tolerance(*base, gx, gy, 0)
    r, flags = check_pass(dr, hk, ctx, st_b, W, H, bg, PASS_SEED, 4, 0, base, tolerance=tol)
    asks, few, noisy = ac.asks(*base, gx, gy, 0, tolerance=tol)
    assert few.any() and noisy.any() and np.array_equal(flags != 0, ac.tiles_of(few | noisy, gx, gy).any(axis=1)) and 0 < r["active_tiles"] < r["tiles"]
    # the planes a pass leaves are planes like any others: back into the first view
    acc, hist, m2 = dp.peek(ctx)
    scene = hk.Scene(path, "")
    counts = ctx.reproject(st_b, st, W, H, 1)
    want = hk.reproject(acc, hist, 1, st_b, st, scene.aov(st_b, W, H), scene.aov(st, W, H), m2=m2)
    got = dp.peek(ctx)
    assert counts == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[3])


def test_what_a_pass_leaves_alone(dr, hk, ctx, tmp_path):
    sc = _load(dr, _cube(tmp_path))
    st, bg, W, H = dr.pack_settings13(sc.settings(), 1), sc.settings().background, 136, 96
    gx, gy = ac.grid(st, W, H)
    fresh = dr.Context(0)
    try:
        fresh.upload(sc)
        fresh.accum_reset(W, H)
        fresh.render_accumulate(st, W, H, bg, 77, STRIDE, 6)
        want = fresh.accum_read()
    finally:
        fresh.close()
    ctx.upload(sc)
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, BASE_SEED, STRIDE, 4)
    base = dp.peek(ctx)
    names = ("kernel", "traversal", "pipe_group", "batch_frames", "feedback", "sky_tiles", "moments", "camera_cert", "camera_entry", "short_one_queue")
    opts, sky, order = {k: ctx.get_option(k) for k in names}, ctx.sky_tiles(), ctx.tile_order()
    stats = ctx.stats()
    tol = _median_tolerance(*base, gx, gy, 4)
    r = ctx.render_adaptive(st, W, H, bg, PASS_SEED, STRIDE, 3, 4, tolerance=tol)
    after = ctx.stats()
    assert after["frames"] == stats["frames"] and after["launches"] == stats["launches"] + 1
    assert after["samples"] == stats["samples"] + r["samples_added"] * int(np.ceil(st[10])) and 0 < r["active_tiles"] < r["tiles"]
    assert {k: ctx.get_option(k) for k in names} == opts and ctx.sky_tiles() == sky
    now = ctx.tile_order()
    assert order is not None and sorted(now) == sorted(order) and all(np.array_equal(now[k], order[k]) for k in order)
    # present and error honour the per-pixel counts
    acc, hist, m2 = dp.peek(ctx)
    assert set(np.unique(hist)) == {0, 3}
    assert np.array_equal(ctx.accum_present(4), pc.present(acc, hist, 4))
    res = ctx.error(st, W, H, 4, tol, sigma=True)
    sig, want_res = hk.error(acc, hist, m2, st, 4, tol)
    got_sig = res.pop("sigma")
    assert res == want_res and np.array_equal(got_sig.view(np.uint32), sig.view(np.uint32))
    _, sig_np = ac.sigma(acc, hist, m2, gx, gy, 4)
    assert np.array_equal(got_sig[:8 * gy, :8 * gx].view(np.uint32), np.ascontiguousarray(sig_np.T).view(np.uint32))
    # the next ordinary render of the view is a fresh context's
    ctx.set_option("moments", 0)
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, 77, STRIDE, 6)
    assert np.array_equal(ctx.accum_read(), want)


def test_render_until_adaptive_is_its_loop(dr, ctx, tmp_path):
    sc = _load(dr, _cube(tmp_path))
    ctx.upload(sc)
    st, bg, W, H = dr.pack_settings13(sc.settings(), 1), sc.settings().background, 136, 96
    gx, gy = ac.grid(st, W, H)
    permille, max_frames = 20, 48
    # the tolerance: the median over tiles of the tile-maximum sigma after the eight uniform frames, so that the first pass's mask is partial
    ctx.accum_reset(W, H)
    ctx.render_accumulate_pipelined(st, W, H, bg, 5, STRIDE, 8)
    tol = _median_tolerance(*dp.peek(ctx), gx, gy, 8)
    ctx.accum_reset(W, H)
    uniform, passes, samples, result = ctx.render_until_adaptive(st, W, H, bg, 5, STRIDE, tol, permille, max_frames, check_every=8, tile_pixels=2)
    got = dp.peek(ctx)
    # by hand: max(4 - 0, 0) -> 8 uniform frames, then passes of 8 with consecutive seeds, judged with the uniform count
    ctx.accum_reset(W, H)
    ctx.render_accumulate_pipelined(st, W, H, bg, 5, STRIDE, 8)
    res, n, added, frames = ctx.error(st, W, H, 8, tol), 0, 0, 8
    while not dr.Context.converged(res, permille) and frames < max_frames:
        r = ctx.render_adaptive(st, W, H, bg, 5 + frames * STRIDE, STRIDE, 8, 8, tolerance=tol, tile_pixels=2)
        n, frames, added = n + 1, frames + 8, added + r["samples_added"]
        if r["active_tiles"] == 0:
            break
        res = ctx.error(st, W, H, 8, tol)
    print("adaptive: tolerance %g, %d uniform frames, %d passes, %d samples added (%.1f frames' worth), %s" % (tol, uniform, passes, samples, samples / (136 * 96), result))
    assert (uniform, passes, samples, result) == (8, n, added, res) and passes >= 1
    assert all(np.array_equal(a, b) for a, b in zip(dp.peek(ctx), got))
    assert samples < passes * 8 * 136 * 96, "every pass rendered every tile: the case does not test what it is for"
    # tolerance 0, no cap, every tile active in every pass (asserted): render_until's sums and M2, and its image at the uniform count
    ctx.accum_reset(W, H)
    frames, res_u = ctx.render_until(st, W, H, bg, 5, STRIDE, 0.0, 0, 24, check_every=8)
    want = (ctx.accum_read(), ctx.accum_moments(), ctx.accum_present(frames))
    ctx.accum_reset(W, H)
    uniform, passes, samples, res_a = ctx.render_until_adaptive(st, W, H, bg, 5, STRIDE, 0.0, 0, 24, check_every=8, max_samples=0)
    assert (frames, uniform, passes, samples) == (24, 8, 2, 2 * 8 * 136 * 96)
    assert np.array_equal(ctx.accum_read(), want[0]) and np.array_equal(ctx.accum_moments(), want[1]) and np.array_equal(ctx.accum_present(uniform), want[2])
    assert {k: res_a[k] for k in ("pixels", "estimated")} == {k: res_u[k] for k in ("pixels", "estimated")}


def test_cli_adaptive(dr, ctx, tmp_path):
    path = _cube(tmp_path)
    exe = os.path.join(ROOT, "dogeray_amd", "bin", "dogeray")
    sc = _load(dr, path)
    ctx.upload(sc)
    for tol, permille, max_frames in ((3.0, 5, 40), (0.0, 0, 16)):
        r = subprocess.run(["timeout", "-k", "10", "120", exe, path, "--quiet", "--until-sigma", "%r,%d" % (tol, permille), "--adaptive", "--max-frames", str(max_frames)],
                           capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        m = re.search(r"^(converged|not converged) after (\d+) frames: (\d+) of (\d+) pixels above (\S+); adaptive: (\d+) uniform frames, (\d+) samples added$", r.stdout, re.M)
        assert m, r.stdout
        pr = dr.ProgressiveRenderer(ctx, sc.settings())
        for _ in range(4):
            td, div = pr.step()
        it = pr.iter
        uniform, passes, samples, result = pr.run_until_adaptive(tol, permille, max_frames)
        print("adaptive CLI: %s; run_until_adaptive %d uniform, %d passes, %d samples" % (m.group(0), uniform, passes, samples))
        assert (int(m.group(3)), int(m.group(4)), int(m.group(6)), int(m.group(7))) == (result["above"], result["pixels"], uniform, samples)
        assert int(m.group(2)) == min(uniform + 8 * passes, max_frames) and (m.group(1) == "converged") == dr.Context.converged(result, permille)
        assert pr.iter == it + uniform and uniform == 8


def test_errors(dr, ctx, tmp_path):
    sc = _load(dr, _cube(tmp_path))
    st, bg, W, H = dr.pack_settings13(sc.settings(), 1), sc.settings().background, 136, 96

    def refused(c, match, *args, **params):
        with pytest.raises(dr.DogerayError, match=match) as e:
            c.render_adaptive(*args, **params)
        assert e.value.code == dr.ERR_INVALID, match

    empty = dr.Context(0)
    try:
        refused(empty, "no scene", st, W, H, bg, 1, STRIDE, 2, 4)
        empty.upload(sc)
        refused(empty, "accum_reset", st, W, H, bg, 1, STRIDE, 2, 4)
        empty.accum_reset(W, H)
        refused(empty, "no moments plane", st, W, H, bg, 1, STRIDE, 2, 4)
        assert len(empty.adaptive_tiles()) == 0
    finally:
        empty.close()
    ctx.upload(sc)
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, bg, 3, STRIDE, 4)
    base = dp.peek(ctx)
    bad = st.copy()
    bad[11] = 0
    refused(ctx, "accum_reset", st, 128, H, bg, 1, STRIDE, 2, 4)
    refused(ctx, "accum_reset", st, W, 95, bg, 1, STRIDE, 2, 4)
    refused(ctx, "nframes", st, W, H, bg, 1, STRIDE, 0, 4)
    refused(ctx, "divide_by", st, W, H, bg, 1, STRIDE, 2, -1)
    refused(ctx, "divisor", bad, W, H, bg, 1, STRIDE, 2, 4)
    for params, msg in (({"tolerance": -0.5}, "tolerance"), ({"tolerance": float("nan")}, "tolerance"), ({"min_samples": 1}, "min_samples"),
                        ({"max_samples": 4}, "max_samples"), ({"tile_pixels": 0}, "tile_pixels"), ({"tile_pixels": 65}, "tile_pixels")):
        refused(ctx, msg, st, W, H, bg, 1, STRIDE, 2, 4, **params)
    ctx.set_stripe(2, 1)
    refused(ctx, "stripe", st, W, H, bg, 1, STRIDE, 2, 4)
    ctx.set_stripe(1, 0)
    ctx.set_option("kernel", 0)
    refused(ctx, "persistent", st, W, H, bg, 1, STRIDE, 2, 4)
    ctx.set_option("kernel", 1)
    ctx.set_traversal(1)
    refused(ctx, "persistent", st, W, H, bg, 1, STRIDE, 2, 4)
    ctx.set_traversal(2)
    # none of the refused calls touched a plane -- or made a history plane
    assert all(np.array_equal(a, b) for a, b in zip(dp.peek(ctx), base)) and base[2].any()
    ptrs = dp.pointers(dr, ctx)
    assert ptrs["hist"][0] is None and ptrs["hist"][1] == 0
