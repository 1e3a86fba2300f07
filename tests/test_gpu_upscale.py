"""The AOV-guided upsampler on the GPU (dr_accum_upscale / Context.upscale, ProgressiveRenderer.image(upscale=...), dogeray --preview): bit for bit
the host build of the same device functions (tools/host_kernel.cpp hk_upscale) on the same accumulator and guides, with a history plane and behind
the a-trous prefilter; the guide caches, what the call leaves alone, its ordering and errors; image quality against the reference's block fill."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import CUBE_SETTINGS, ROOT, SCENES, with_settings
import denoise_checks as dc

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))

SWITCHES = ({}, {"demodulate": 0}, {"material_stop": 0}, {"sigma_depth": 0.0, "normal_power_log2": 0}, {"normal_power_log2": 16})
# guided MSE / block-fill MSE against a 4096-frame full-resolution mean, 256x256, div 2, 4 frames: the ratio measured on an MI355X (cube 0.490,
# matball 0.597) x 1.25 (the seed-to-seed variation of a 256x256 image), rounded up to one decimal and never above 0.9
QUALITY_BOUND = {"cube": 0.7, "matball": 0.8}


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
def paths(synth, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("upscale_gpu")
    cube = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp / "cube.rts"), CUBE_SETTINGS)
    textest = os.path.join(SCENES, "textest.rts")
    if not any(l.startswith("*") for l in open(textest)):
        textest = with_settings(textest, str(tmp / "textest.rts"), CUBE_SETTINGS)
    return {"cube": (cube, 136, 96), "matball": (os.path.join(synth["dir"], "matball.rts"), 120, 88), "textest": (textest, 136, 96),
            "hf_small": (os.path.join(synth["dir"], "hf_small.rts"), 160, 96)}


_guides = {}


def _host(hk, path, acc, st, divide_by, **kw):
    """hk_upscale fed with the host build's own AOVs of both grids (traced once per view)"""
    W, H = acc.shape[0], acc.shape[1]
    full13 = np.array(st, np.float32)
    full13[11] = 1
    g = []
    for s13 in (st, full13):
        key = (path, W, H, np.asarray(s13, np.float32).tobytes())
        if key not in _guides:
            _guides[key] = hk.Scene(path, "").aov(s13, W, H)
        g.append(_guides[key])
    f, rgb, _ = hk.upscale(acc, st, divide_by, g[0], g[1], **kw)
    return f, rgb


def _load(dr, path):
    sc = dr.Scene.load(path, "")
    sc.build_bvh()
    return sc


def _render(ctx, sc, st, W, H, frames, seed=3):
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, sc.settings().background, seed, 1000003, frames)
    return ctx.accum_read()


def _same(got, want, what):
    f, r = got
    wf, wr = want
    assert dc.same_bits(f, wf), "%s: f32 differs at %d values" % (what, int((dc.bits(f) != dc.bits(wf)).sum()))
    assert np.array_equal(r, wr), what


@pytest.mark.parametrize("mode", [2, 0, 1])
def test_gpu_equals_the_host_build(dr, hk, ctx, paths, mode):
    for name, (path, W, H) in paths.items():
        sc = _load(dr, path)
        ctx.upload(sc)
        ctx.set_traversal(mode)
        for div in (2, 4, 8):
            st = dr.pack_settings13(sc.settings(), div)
            acc = _render(ctx, sc, st, W, H, 3)
            sets = [{}] if mode != 2 else list(SWITCHES) + [{"mode": dr.UPSCALE_BLOCK}]
            for params in sets:
                what = "%s div %d traversal %d %s" % (name, div, mode, params)
                want = _host(hk, path, acc, st, 3, **params)
                rgb, f = ctx.upscale(st, W, H, 3, out="both", **params)
                _same((f, rgb), want, what)
                assert f[:, :W // div // 8 * 8 * div].any() and not f[:, W // div // 8 * 8 * div:].any() and not f[H // div // 8 * 8 * div:].any(), what
                if params in ({}, {"mode": dr.UPSCALE_BLOCK}):
                    rgb, f = ctx.upscale(st, W, H, 3, out="both", device=True, **params)
                    assert rgb.is_cuda and f.is_cuda and tuple(f.shape) == (H, W, 3)
                    _same((f.cpu().numpy(), rgb.cpu().numpy()), want, what + " device tensors")
                    _same((ctx.upscale(st, W, H, 3, out="f32", **params), ctx.upscale(st, W, H, 3, **params)), want, what + " one output")
        if mode == 2:                        # div 1, block: dr_accum_present byte for byte
            st = dr.pack_settings13(sc.settings(), 1)
            _render(ctx, sc, st, W, H, 2)
            assert np.array_equal(ctx.upscale(st, W, H, 2, mode=dr.UPSCALE_BLOCK), ctx.accum_present(2)), name
    ctx.set_traversal(2)


def test_history_plane(dr, hk, ctx, paths):
    path, W, H = paths["hf_small"]
    sc = _load(dr, path)
    ctx.upload(sc)
    s = sc.settings()
    st_a = dr.pack_settings13(s, 2)
    st_b = st_a.copy()
    st_b[0] += 0.3
    _render(ctx, sc, st_a, W, H, 3)
    counts = ctx.reproject(st_a, st_b, W, H, 3)
    assert counts["valid"] > 0
    ctx.render_accumulate(st_b, W, H, s.background, 50, 1000003, 2)
    acc, hist = ctx.accum_read(), ctx.accum_history()
    assert (hist > 0).any() and (hist == 0).any()
    for params in ({}, {"mode": dr.UPSCALE_BLOCK}):
        _same(ctx.upscale(st_b, W, H, 2, out="both", **params)[::-1], _host(hk, path, acc, st_b, 2, hist=hist, **params), "history %s" % params)
    _same(ctx.upscale(st_b, W, H, 2, out="both", prefilter={"iterations": 2})[::-1],
          _host(hk, path, acc, st_b, 2, hist=hist, prefilter={"iterations": 2}), "history, prefilter")
    ctx.accum_reset(W, H)


def test_prefilter(dr, hk, ctx, paths):
    for name in ("cube", "matball"):
        path, W, H = paths[name]
        sc = _load(dr, path)
        ctx.upload(sc)
        st = dr.pack_settings13(sc.settings(), 2)
        acc = _render(ctx, sc, st, W, H, 3)
        for tiles in (1, 0):
            ctx.set_option("denoise_tiles", tiles)
            for pre in (True, {"iterations": 1}, {"iterations": 3, "sigma_luminance": 2.5}):
                want = _host(hk, path, acc, st, 3, prefilter={} if pre is True else pre)
                _same(ctx.upscale(st, W, H, 3, out="both", prefilter=pre)[::-1], want, "%s tiles %d prefilter %s" % (name, tiles, pre))
        ctx.set_option("denoise_tiles", 1)
        want = _host(hk, path, acc, st, 3, demodulate=0, prefilter={"demodulate": 0})
        _same(ctx.upscale(st, W, H, 3, out="both", demodulate=0, prefilter=True)[::-1], want, "%s demodulate 0" % name)
    # the second-moment plane: the prefilter's variance is the temporal one where a pixel has four samples
    ctx.set_option("moments", 1)
    try:
        acc = _render(ctx, sc, st, W, H, 6)
        m2 = ctx.accum_moments()
        ctx.set_option("denoise_variance", 1)
        got = ctx.upscale(st, W, H, 6, out="both", prefilter=True)[::-1]
        _same(got, _host(hk, path, acc, st, 6, m2=m2, prefilter={}), "moments")
        assert not dc.same_bits(got[0], _host(hk, path, acc, st, 6, prefilter={})[0])
    finally:
        ctx.set_option("denoise_variance", 0)
        ctx.set_option("moments", 0)
        ctx.accum_reset(W, H)


def test_guide_caches(dr, hk, paths):
    path, W, H = paths["cube"]
    sc = _load(dr, path)
    c = dr.Context(0)
    try:
        c.upload(sc)
        st2, st4 = dr.pack_settings13(sc.settings(), 2), dr.pack_settings13(sc.settings(), 4)
        acc = _render(c, sc, st2, W, H, 2)
        passes = lambda: c.get_option("upscale_aov_passes")
        assert passes() == 0
        c.upscale(st2, W, H, 2, mode=dr.UPSCALE_BLOCK)
        assert passes() == 0                      # block mode traces nothing
        want = _host(hk, path, acc, st2, 2)
        _same(c.upscale(st2, W, H, 2, out="both")[::-1], want, "first call")
        assert passes() == 2
        c.upscale(st4, W, H, 2)
        assert passes() == 1                      # the same view at another divisor: the full-resolution guides are kept
        c.upscale(st4, W, H, 2)
        assert passes() == 0
        # the denoiser's cache is the low side's: its bits with an upscale in between are the bits without one, and it leaves the low guides warm
        d0 = c.denoise(st2, W, H, 2, out="f32")
        _same(c.upscale(st2, W, H, 2, out="both")[::-1], want, "after a denoise of the same settings")
        assert passes() == 0
        c.upscale(st4, W, H, 2, prefilter=True)
        assert passes() == 1
        d1 = c.denoise(st2, W, H, 2, out="f32")
        a = hk.Scene(path, "").aov(st2, W, H)
        dwant = hk.denoise(acc, st2, 2, a["normal"], a["albedo"], a["depth"], a["material"])[0]
        assert dc.same_bits(d0, d1) and dc.same_bits(d0, dwant)
        moved = st2.copy()
        moved[0] += 0.5
        c.upscale(moved, W, H, 2)
        assert passes() == 2
        _same(c.upscale(st2, W, H, 2, out="both")[::-1], want, "back to the first view")
        assert passes() == 2
        c.upload(sc)
        _same(c.upscale(st2, W, H, 2, out="both")[::-1], want, "after an upload")
        assert passes() == 2
    finally:
        c.close()


def test_ordering_and_what_it_leaves_alone(dr, hk, ctx, paths, tmp_path):
    path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube256.rts"), CUBE_SETTINGS)
    sc = _load(dr, path)
    ctx.upload(sc)
    s = sc.settings()
    st = dr.pack_settings13(s, 2)
    W, H = 256, 256
    ctx.accum_reset(W, H)
    # ordered behind dr_pipeline_submit: the call sees every frame submitted before it
    tickets = [ctx.pipeline_submit(st, W, H, s.background, 11 + 1000003 * k, present_divide_by=k + 1) for k in range(3)]
    got = ctx.upscale(st, W, H, 3, out="both")
    for t in tickets:
        ctx.pipeline_wait(t)
    acc = ctx.accum_read()
    assert acc.any()
    _same(got[::-1], _host(hk, path, acc, st, 3), "behind the pipeline")
    # leaves the accumulator, its history, the statistics and the options alone
    names = ("kernel", "traversal", "pipe_group", "batch_frames", "denoise_tiles", "denoise_variance", "moments", "camera_cert")
    opts = {k: ctx.get_option(k) for k in names}
    before, hist = ctx.stats(), ctx.accum_history()
    ctx.upscale(st, W, H, 3)
    ctx.upscale(st, W, H, 3, out="f32", device=True, prefilter=True)
    ctx.upscale(st, W, H, 3, mode=dr.UPSCALE_BLOCK)
    assert np.array_equal(ctx.accum_read(), acc) and np.array_equal(ctx.accum_history(), hist) and ctx.stats() == before
    assert {k: ctx.get_option(k) for k in names} == opts


def test_upscale_errors(dr, ctx, tmp_path):
    st0 = np.zeros(13, np.float32) + 1
    path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "c.rts"), CUBE_SETTINGS)
    sc = _load(dr, path)
    empty = dr.Context(0)
    try:
        with pytest.raises(dr.DogerayError, match="no scene"):
            empty.upscale(st0, 64, 64, 1)
        empty.upload(sc)
        st = dr.pack_settings13(sc.settings(), 2)
        with pytest.raises(dr.DogerayError, match="accumulator"):
            empty.upscale(st, 256, 256, 1)
        assert empty.get_option("upscale_aov_passes") == 0
    finally:
        empty.close()
    ctx.upload(sc)
    ctx.accum_reset(256, 256)
    ctx.render_accumulate(st, 256, 256, sc.settings().background, 1, 1000003, 1)
    ok = (st, 256, 256, 1)
    cases = [((st, 128, 256, 1), {}), ((st, 256, 255, 1), {}), ((st, 256, 256, 0), {}), ((st, 256, 256, -3), {}),
             (ok, {"mode": 2}), (ok, {"mode": -1}), (ok, {"normal_power_log2": 17}), (ok, {"normal_power_log2": -1}), (ok, {"sigma_depth": -0.01}),
             (ok, {"sigma_depth": float("nan")}), (ok, {"prefilter": {"iterations": 0}}), (ok, {"prefilter": {"iterations": 11}}),
             (ok, {"prefilter": {"demodulate": 0}}), (ok, {"prefilter": {"sigma_luminance": -1.0}}), (ok, {"prefilter": True, "mode": 0}),
             (ok, {"prefilter": {"demodulate": 1}, "demodulate": 0})]
    bad = st.copy()
    bad[11] = 0
    cases.append(((bad, 256, 256, 1), {}))
    for args, params in cases:
        for device in (False, True):
            with pytest.raises(dr.DogerayError) as e:
                ctx.upscale(*args, device=device, **params)
            assert e.value.code == dr.ERR_INVALID and str(e.value), (args[1:], params)
    p = dr.upscale_params()
    rc = dr.lib().dr_accum_upscale(ctx._h, st.ctypes.data_as(C.c_void_p), 256, 256, 1, C.byref(p), None, None, None, 0)
    assert rc == dr.ERR_INVALID and "no output" in dr.lib().dr_last_error().decode()
    with pytest.raises(ValueError):
        ctx.upscale(st, 256, 256, 1, out="png")
    with pytest.raises(TypeError):
        ctx.upscale(st, 256, 256, 1, sigma=3)
    # params NULL: the defaults
    got = np.empty((256, 256, 3), np.uint8)
    assert dr.lib().dr_accum_upscale(ctx._h, st.ctypes.data_as(C.c_void_p), 256, 256, 1, None, None, None, got.ctypes.data_as(C.c_void_p), 0) == 0
    assert np.array_equal(got, ctx.upscale(st, 256, 256, 1))
    # a divisor that leaves no grid: zeros
    none = dr.pack_settings13(sc.settings(), 64)
    assert not ctx.upscale(none, 256, 256, 1, out="f32").any()


def test_progressive_renderer_shows_the_ladder_at_full_size(dr, hk, ctx, synth):
    path = os.path.join(synth["dir"], "hf_small.rts")
    sc = _load(dr, path)
    ctx.upload(sc)
    pr = dr.ProgressiveRenderer(ctx, sc.settings(), seed_base=7)
    W, H = pr.W, pr.H
    for k in range(4):                         # the preview ladder: div 8, 4, 2, 1
        td, div = pr.step()
        st = pr.settings13()
        assert int(st[11]) == td == dr.ProgressiveRenderer.LADDER[k]
        acc = ctx.accum_read()
        want = _host(hk, path, acc, st, div)
        img = pr.image(div, upscale=True)
        assert np.array_equal(img, ctx.upscale(st, W, H, div)) and np.array_equal(img, want[1]), "ladder step %d" % k
        blk = pr.image(div, upscale={"mode": dr.UPSCALE_BLOCK})
        present = ctx.accum_present(div)
        g = (W // td // 8 * 8, H // td // 8 * 8)
        assert np.array_equal(blk[:g[1] * td, :g[0] * td], np.repeat(np.repeat(present[:g[1], :g[0]], td, axis=0), td, axis=1)), "ladder step %d" % k
        assert np.array_equal(pr.image(div, denoise={"iterations": 2}, upscale=True), ctx.upscale(st, W, H, div, prefilter={"iterations": 2}))
        assert np.array_equal(pr.image(div), present) and np.array_equal(pr.image(div, upscale=None), present)
        assert np.array_equal(pr.image(div, denoise=True), ctx.denoise(st, W, H, div))


def _read_bmp(path, W, H):
    data = open(path, "rb").read()
    assert data[:2] == b"BM" and len(data) == 122 + W * H * 4
    bgra = np.frombuffer(data, np.uint8, offset=122).reshape(H, W, 4)[::-1]
    return np.ascontiguousarray(bgra[..., 2::-1])


@pytest.mark.parametrize("block", [False, True])
def test_cli_writes_the_previews(dr, ctx, tmp_path, block):
    path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube.rts"), CUBE_SETTINGS)
    exe = os.path.join(ROOT, "dogeray_amd", "bin", "dogeray")
    prefix = str(tmp_path / "pre")
    r = subprocess.run(["timeout", "-k", "10", "120", exe, path, "--frames", "1", "--quiet", "--preview", prefix] + (["--preview-block"] if block else []),
                       capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    sc = _load(dr, path)
    ctx.set_traversal(2)
    ctx.upload(sc)
    pr = dr.ProgressiveRenderer(ctx, sc.settings())
    for td in (8, 4, 2):
        assert "exported preview:%s_%d.bmp" % (prefix, td) in r.stdout
        _, div = pr.step()
        want = pr.image(div, upscale={"mode": dr.UPSCALE_BLOCK} if block else True)
        assert want.any() and np.array_equal(_read_bmp("%s_%d.bmp" % (prefix, td), pr.W, pr.H), want), td
    assert not os.path.exists(prefix + "_1.bmp")


@pytest.mark.parametrize("name", ["cube", "matball"])
def test_quality_against_the_block_fill(dr, ctx, synth, tmp_path, name):
    """256x256, 4 frames at div 2: against a 4096-frame full-resolution mean the guided image's MSE is below the block fill's of the same
    accumulator (the reference's display), by the bound above"""
    path = os.path.join(synth["dir"], "matball.rts") if name == "matball" else with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "c.rts"), CUBE_SETTINGS)
    sc = _load(dr, path)
    ctx.upload(sc)
    W, H = 256, 256
    st1, st2 = dr.pack_settings13(sc.settings(), 1), dr.pack_settings13(sc.settings(), 2)
    ref = _render(ctx, sc, st1, W, H, 4096, seed=1000).astype(np.float64).transpose(1, 0, 2) / 4096
    _render(ctx, sc, st2, W, H, 4, seed=77)
    guided = ctx.upscale(st2, W, H, 4, out="f32").astype(np.float64)
    block = ctx.upscale(st2, W, H, 4, out="f32", mode=dr.UPSCALE_BLOCK).astype(np.float64)
    mse_g, mse_b = float(((guided - ref) ** 2).mean()), float(((block - ref) ** 2).mean())
    print("upscale quality %s: MSE block %.3f guided %.3f ratio %.3f" % (name, mse_b, mse_g, mse_g / mse_b))
    assert mse_g < mse_b and mse_g <= QUALITY_BOUND[name] * mse_b, (mse_b, mse_g)
