"""Lens-averaged AOVs on the GPU (dr_render_aov_lens / Context.render_aov_lens, option guide_frames): bit for bit the fold of the public pieces
(Context.kat_camera rays through Context.trace, tests/aov_lens_checks.py) and the host build of the same per-pixel body (hk_aov_lens), with every
traversal and loop shape; windows and device tensors; the denoiser and the upscaler guided by them against the host build fed the same guides; the
guide cache across changes of the option; the refusals; and what the feature is for: a defocused image denoised better than with pinhole guides."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
import aov_lens_checks as lc

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

NFRAMES, SPP, APERTURE = 3, 2, 0.5


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


@pytest.fixture(scope="module")
def scenes(dr, hk, synth, tmp_path_factory):
    """name -> (path, the loaded scene, the host build's scene, settings13 with the tests' aperture and spp)"""
    out = {}
    for name, path in lc.scene_paths(synth, tmp_path_factory.mktemp("lens")):
        sc = dr.Scene.load(path, "")
        sc.build_bvh()
        out[name] = (path, sc, hk.Scene(path, ""), lc.lens_settings(dr.pack_settings13(sc.settings(), 1), APERTURE, SPP))
    return out


@pytest.fixture(scope="module")
def folds(ctx, scenes):
    """the definition over the window, from the public pieces on the GPU: computed once per scene"""
    out = {}
    ctx.set_traversal(2)
    for name, (path, sc, hsc, st) in scenes.items():
        ctx.upload(sc)
        out[name] = lc.fold(ctx.kat_camera, ctx.trace, st, lc.W, lc.H, lc.WINDOW, lc.SEED, lc.STRIDE, NFRAMES)
    return out


@pytest.mark.parametrize("mode", [2, 0, 1])
def test_definition_from_public_pieces_and_the_host_build(ctx, scenes, folds, mode):
    for name, (path, sc, hsc, st) in scenes.items():
        ctx.upload(sc)
        ctx.set_traversal(mode)
        got = ctx.render_aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, NFRAMES, window=lc.WINDOW)
        lc.assert_same(got, folds[name], "%s traversal %d: the fold of kat_camera through trace" % (name, mode))
        lc.assert_same(got, hsc.aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, NFRAMES, window=lc.WINDOW), "%s traversal %d: host build" % (name, mode))
        lc.check_properties(got, name)
        part = (got["coverage"] > 0) & (got["coverage"] < 1)
        assert part.any(), "%s: no pixel is partly covered" % name
    ctx.set_traversal(2)


def test_sample_counts_at_both_ends(ctx, scenes):
    """N = 256 on one 8x8 window, N = 1 and a seed that wraps, against the host build, with both loop shapes"""
    path, sc, hsc, st = scenes["matball"]
    ctx.upload(sc)
    win = (32, 24, 8, 8)
    st1 = lc.lens_settings(st, APERTURE, 1)
    big = 2 ** 64 - 5                          # frame_seed + k * seed_stride runs past 2^64
    want256 = hsc.aov_lens(st, lc.W, lc.H, 7, 11, 128, window=win)
    want1 = hsc.aov_lens(st1, lc.W, lc.H, 7, 11, 1)
    want_big = hsc.aov_lens(st, lc.W, lc.H, big, 3, NFRAMES, window=win)
    try:
        for loop in (0, 1):
            ctx.set_option("aov_lens_loop", loop)
            lc.assert_same(ctx.render_aov_lens(st, lc.W, lc.H, 7, 11, 128, window=win), want256, "N = 256, loop %d" % loop)
            lc.assert_same(ctx.render_aov_lens(st1, lc.W, lc.H, 7, 11, 1), want1, "N = 1, loop %d" % loop)
            lc.assert_same(ctx.render_aov_lens(st, lc.W, lc.H, big, 3, NFRAMES, window=win), want_big, "wrapping seed, loop %d" % loop)
    finally:
        ctx.set_option("aov_lens_loop", 0)


def test_windows_device_tensors_and_channel_subsets(dr, ctx, scenes):
    path, sc, hsc, st = scenes["cube"]
    ctx.upload(sc)
    full = ctx.render_aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, NFRAMES)
    assert full["coverage"].shape == (lc.H // 8 * 8, lc.W // 8 * 8) and full["normal"].shape == full["coverage"].shape + (3,)
    x0, y0, w, h = lc.WINDOW
    win = ctx.render_aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, NFRAMES, window=lc.WINDOW)
    lc.assert_same(win, {k: np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w]) for k, a in full.items()}, "window")
    dev = ctx.render_aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, NFRAMES, window=lc.WINDOW, device=True)
    assert all(a.is_cuda for a in dev.values())
    lc.assert_same({k: a.cpu().numpy() for k, a in dev.items()}, win, "device tensors")
    some = ctx.render_aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, NFRAMES, window=lc.WINDOW, channels=("material", "albedo"))
    assert sorted(some) == ["albedo", "material"]
    lc.assert_same(some, win, "channel subset", channels=("material", "albedo"))
    with pytest.raises(ValueError):
        ctx.render_aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, NFRAMES, channels=("uv",))


@pytest.mark.parametrize("mode", [2, 0])
def test_loop_shapes_give_the_same_bits(dr, ctx, scenes, mode):
    """the nested loop (the default) and the refilling walk loop (private option aov_lens_loop = 1), against each other and the host build"""
    ctx.set_traversal(mode)
    assert ctx.get_option("aov_lens_loop") == 0
    try:
        for name, (path, sc, hsc, st) in scenes.items():
            ctx.upload(sc)
            got = []
            for loop in (0, 1):
                ctx.set_option("aov_lens_loop", loop)
                got.append(ctx.render_aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, NFRAMES, window=lc.WINDOW))
            lc.assert_same(got[1], got[0], "%s: refilling against nested" % name)
            lc.assert_same(got[1], hsc.aov_lens(st, lc.W, lc.H, lc.SEED, lc.STRIDE, NFRAMES, window=lc.WINDOW), "%s: refilling against the host build" % name)
            assert (got[0]["coverage"] > 0).any()
        with pytest.raises(dr.DogerayError):
            ctx.set_option("aov_lens_loop", 2)
    finally:
        ctx.set_option("aov_lens_loop", 0)
        ctx.set_traversal(2)


def _same_image(got, want, what):
    f, rgb = got
    wf, wrgb = want
    assert np.array_equal(lc.bits(f), lc.bits(wf)), "%s: f32 differs at %d values" % (what, int((lc.bits(f) != lc.bits(wf)).sum()))
    assert np.array_equal(rgb, wrgb), what


def _lens_guides(dr, hsc, st, W, H, frames):
    return hsc.aov_lens(st, W, H, dr.GUIDE_SEED, 1, frames, as_guides=True)


def test_denoise_and_upscale_take_the_lens_guides(dr, hk, ctx, scenes):
    """guide_frames = 4: Context.denoise / upscale equal the host build fed hk_aov_lens's guide form; 0 -> 4 -> 0 traces again each time"""
    path, sc, hsc, st = scenes["matball"]
    ctx.upload(sc)
    W, H = 120, 88
    bg = sc.settings().background
    assert ctx.get_option("guide_frames") == 0
    try:
        ctx.accum_reset(W, H)
        ctx.render_accumulate(st, W, H, bg, 3, 1000003, 3)
        acc = ctx.accum_read()
        passes = lambda: ctx.get_option("upscale_aov_passes")

        def low_guides_are_cached():
            """The denoiser has no pass counter of its own; the upscaler's low side reads the denoiser's guide set (at divisor 1 the same view)
            and counts what it had to trace.  1 = only the upscaler's own full-resolution set: the denoise call before traced the low set under
            the option's current value, or the upscaler would have had to (2)."""
            ctx.upscale(st, W, H, 3)
            return passes() == 1
        first = ctx.denoise(st, W, H, 3, out="both")
        assert low_guides_are_cached()
        ctx.set_option("guide_frames", 4)
        rgb, f = ctx.denoise(st, W, H, 3, out="both")
        assert low_guides_are_cached()             # denoise traced again under 4 (stale pinhole guides would have made the upscaler trace: 2)
        g = _lens_guides(dr, hsc, st, W, H, 4)
        _same_image((f, rgb), hk.denoise(acc, st, 3, g["normal"], g["albedo"], g["depth"], g["material"]), "denoise with lens guides")
        assert not np.array_equal(lc.bits(f), lc.bits(first[1])), "the lens guides change nothing"
        ctx.set_option("guide_frames", 0)
        third = ctx.denoise(st, W, H, 3, out="both")
        assert low_guides_are_cached()             # and again under 0
        assert first[0].tobytes() == third[0].tobytes() and first[1].tobytes() == third[1].tobytes(), "stale guides after 4 -> 0"
        ctx.upscale(st, W, H, 3)
        assert passes() == 0                       # (nothing changed: nothing traced)
        # the upscaler: both guide sets, and the aov-pass counter across the option's changes
        st2 = st.copy()
        st2[11] = 2
        full13 = st.copy()
        full13[11] = 1
        ctx.accum_reset(W, H)
        ctx.render_accumulate(st2, W, H, bg, 5, 1000003, 3)
        acc2 = ctx.accum_read()
        up0 = ctx.upscale(st2, W, H, 3, out="both", prefilter=True)
        assert passes() == 1                      # the low view is new; the full-resolution view is st itself, traced above
        ctx.upscale(st2, W, H, 3, prefilter=True)
        assert passes() == 0
        ctx.set_option("guide_frames", 4)
        urgb, uf = ctx.upscale(st2, W, H, 3, out="both", prefilter=True)
        assert passes() == 2
        want = hk.upscale(acc2, st2, 3, _lens_guides(dr, hsc, st2, W, H, 4), _lens_guides(dr, hsc, full13, W, H, 4), prefilter={})
        _same_image((uf, urgb), want[:2], "upscale with lens guides")
        ctx.upscale(st2, W, H, 3, prefilter=True)
        assert passes() == 0
        ctx.set_option("guide_frames", 0)
        up2 = ctx.upscale(st2, W, H, 3, out="both", prefilter=True)
        assert passes() == 2
        assert up0[0].tobytes() == up2[0].tobytes() and up0[1].tobytes() == up2[1].tobytes(), "stale guides after 4 -> 0"
    finally:
        ctx.set_option("guide_frames", 0)


def test_errors(dr, ctx, scenes):
    path, sc, hsc, st = scenes["cube"]
    ctx.upload(sc)
    for nframes in (0, 129, -2):                                             # N = 0, 258
        with pytest.raises(dr.DogerayError) as e:
            ctx.render_aov_lens(st, lc.W, lc.H, 1, 1, nframes)
        assert e.value.code == dr.ERR_INVALID and "samples" in str(e.value)
    st257 = lc.lens_settings(st, APERTURE, 257)
    with pytest.raises(dr.DogerayError) as e:
        ctx.render_aov_lens(st257, lc.W, lc.H, 1, 1, 1)
    assert e.value.code == dr.ERR_INVALID
    for window in ((70, 0, 8, 8), (0, 0, 0, 8), (-1, 0, 8, 8)):
        for device in (False, True):
            with pytest.raises(dr.DogerayError) as e:
                ctx.render_aov_lens(st, lc.W, lc.H, 1, 1, 1, window=window, device=device)
            assert e.value.code == dr.ERR_INVALID
    empty = dr.Context(0)
    try:
        with pytest.raises(dr.DogerayError, match="no scene") as e:
            empty.render_aov_lens(st, lc.W, lc.H, 1, 1, 1)
        assert e.value.code == dr.ERR_INVALID
        for bad in (-1, 257):
            with pytest.raises(dr.DogerayError):
                empty.set_option("guide_frames", bad)
        assert empty.get_option("guide_frames") == 0
    finally:
        empty.close()
    # guide_frames * spp > 256 is refused by the call that traces
    ctx.accum_reset(lc.W, lc.H)
    ctx.render_accumulate(st, lc.W, lc.H, 1.0, 1, 1000003, 1)
    ctx.set_option("guide_frames", 200)
    try:
        with pytest.raises(dr.DogerayError, match="guide_frames") as e:
            ctx.denoise(st, lc.W, lc.H, 1)
        assert e.value.code == dr.ERR_INVALID
    finally:
        ctx.set_option("guide_frames", 0)
    ctx.denoise(st, lc.W, lc.H, 1)


def test_quality_under_defocus(dr, ctx, tmp_path):
    """What the feature is for.  A checker floor and two spheres, the camera focused on the near one, the far one's circle of confusion >= 4 pixels at
    256x256; the 4-frame accumulator denoised with guide_frames = 16 has a smaller MSE against the 4096-frame mean than with the pinhole guides
    (guide_frames = 0, the behaviour before the option), and at most half the raw mean's."""
    path = lc.defocus_scene(dr, str(tmp_path / "defocus.rts"))
    sc = dr.Scene.load(path, "")
    sc.build_bvh()
    ctx.set_traversal(2)
    ctx.upload(sc)
    st = dr.pack_settings13(sc.settings(), 1)
    W, H = 256, 256
    D = lc.DEFOCUS
    far_depth = D["campos"][2] - D["far"][0][2] - D["far"][1]             # the far sphere's nearest point along the view axis (-z)
    near_depth = D["campos"][2] - D["near"][0][2]
    coc = lc.circle_of_confusion(st, W, far_depth)
    print("defocus: circle of confusion of the far sphere %.2f px, of the near sphere's centre %.2f px" % (coc, lc.circle_of_confusion(st, W, near_depth)))
    assert coc >= 4.0 and lc.circle_of_confusion(st, W, D["focus"]) == 0.0
    bg = sc.settings().background

    def render(frames, seed):
        ctx.accum_reset(W, H)
        ctx.render_accumulate(st, W, H, bg, seed, 1000003, frames)
        return ctx.accum_read().astype(np.float64).transpose(1, 0, 2) / frames
    ref = render(4096, 1000)
    raw = render(4, 77)
    try:
        ctx.set_option("guide_frames", 0)
        pinhole = ctx.denoise(st, W, H, 4, out="f32").astype(np.float64)
        ctx.set_option("guide_frames", 16)
        lens = ctx.denoise(st, W, H, 4, out="f32").astype(np.float64)
    finally:
        ctx.set_option("guide_frames", 0)
    mse = lambda img: float(((img - ref) ** 2).mean())
    mse_raw, mse_pinhole, mse_lens = mse(raw), mse(pinhole), mse(lens)
    print("defocus quality: MSE raw %.3f pinhole guides %.3f lens guides %.3f; lens / pinhole %.3f, lens / raw %.3f"
          % (mse_raw, mse_pinhole, mse_lens, mse_lens / mse_pinhole, mse_lens / mse_raw))
    # measured: raw 249.8, pinhole guides 948.2, lens guides 61.2 -- lens / pinhole 0.065; the bound is halfway between that and 1, so that the
    # seed-to-seed scatter of a 4-frame input cannot flip it
    assert mse_lens < mse_pinhole and mse_lens <= 0.53 * mse_pinhole, (mse_raw, mse_pinhole, mse_lens)
    assert mse_lens <= 0.5 * mse_raw, (mse_raw, mse_lens)
