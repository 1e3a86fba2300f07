"""The a-trous denoiser on the GPU (dr_accum_denoise / Context.denoise, ProgressiveRenderer.image(denoise=...), dogeray --denoise): bit for bit the
host build of the same device functions (tools/host_kernel.cpp hk_denoise) on the same accumulator and guides, image quality against a long
mean, the guide cache, ordering behind the pipeline, what it leaves alone, and its errors."""
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


def _load(dr, path):
    sc = dr.Scene.load(path, "")
    sc.build_bvh()
    return sc


def _render(ctx, sc, st, W, H, frames, seed=3):
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, sc.settings().background, seed, 1000003, frames)
    return ctx.accum_read()


def _host(hk, path, acc, st, div, **params):
    W, H = acc.shape[0], acc.shape[1]
    a = hk.Scene(path, "").aov(st, W, H)
    return hk.denoise(acc, st, div, a["normal"], a["albedo"], a["depth"], a["material"], **params)


def _same(got, want, what):
    f, r = got
    wf, wr = want
    assert dc.same_bits(f, wf), "%s: f32 differs at %d values" % (what, int((dc.bits(f) != dc.bits(wf)).sum()))
    assert np.array_equal(r, wr), what


@pytest.mark.parametrize("mode", [2, 0, 1])
def test_gpu_equals_the_host_build(dr, hk, ctx, synth, tmp_path, mode):
    for name, path, W, H in _cases(synth, tmp_path):
        sc = _load(dr, path)
        ctx.upload(sc)
        ctx.set_traversal(mode)
        st = dr.pack_settings13(sc.settings(), 1)
        acc = _render(ctx, sc, st, W, H, 3)
        sets = [{}] if mode != 2 else [{"iterations": i} for i in range(6)] + [{"demodulate": 0}, {"material_stop": 0}, {"iterations": 10}]
        for params in sets:
            for tiles in ((1, 0) if mode == 2 else (1,)):
                ctx.set_option("denoise_tiles", tiles)
                rgb, f = ctx.denoise(st, W, H, 3, out="both", **params)
                _same((f, rgb), _host(hk, path, acc, st, 3, **params), "%s traversal %d %s tiles %d" % (name, mode, params, tiles))
        ctx.set_option("denoise_tiles", 1)
        # the restatement, once per scene
        a = hk.Scene(path, "").aov(st, W, H)
        _same((ctx.denoise(st, W, H, 3, out="f32"), ctx.denoise(st, W, H, 3)),
              dc.denoise(acc, st, 3, a["normal"], a["albedo"], a["depth"], a["material"]), "%s: restatement" % name)
        # iterations 0: dr_accum_present byte for byte
        assert np.array_equal(ctx.denoise(st, W, H, 3, iterations=0), ctx.accum_present(3)), name
    ctx.set_traversal(2)


def test_device_tensors_and_preview_ladder(dr, hk, ctx, synth):
    import torch
    path = os.path.join(synth["dir"], "hf_small.rts")
    sc = _load(dr, path)
    ctx.upload(sc)
    pr = dr.ProgressiveRenderer(ctx, sc.settings(), seed_base=7)
    W, H = pr.W, pr.H
    for k in range(4):                         # the preview ladder: div 8, 4, 2, 1
        td, div = pr.step()
        st = pr.settings13()
        assert int(st[11]) == dr.ProgressiveRenderer.LADDER[k]
        acc = ctx.accum_read()
        want = _host(hk, path, acc, st, div)
        assert np.array_equal(pr.image(div, denoise=True), want[1]), "ladder step %d" % k
        assert np.array_equal(pr.image(div), ctx.accum_present(div)) and np.array_equal(pr.image(div, denoise={"iterations": 0}), ctx.accum_present(div))
        rgb, f = ctx.denoise(st, W, H, div, out="both", device=True)
        side = torch.zeros(1, device="cuda:0")
        side += f.sum() * 0                     # consumed on torch's stream right away
        assert rgb.is_cuda and f.is_cuda and tuple(f.shape) == (H, W, 3)
        _same((f.cpu().numpy(), rgb.cpu().numpy()), want, "ladder step %d, device tensors" % k)
    pr.step()
    st = pr.settings13()
    assert int(st[11]) == 1 and pr.iter == 5
    f = ctx.denoise(st, W, H, 2, out="f32", device=True, sigma_luminance=2.5, normal_power_log2=3)
    _same((f.cpu().numpy(), ctx.denoise(st, W, H, 2, sigma_luminance=2.5, normal_power_log2=3)),
          _host(hk, path, ctx.accum_read(), st, 2, sigma_luminance=2.5, normal_power_log2=3), "device f32")


def test_full_size_c4(dr, hk):
    """The 1M-triangle C4 stand-in at 1920x1080: the GPU equals hk_denoise fed with the GPU's own AOVs"""
    sys.path.insert(0, ROOT)
    import bench
    path = bench.ensure_scene(os.environ.get("DOGERAY_BENCH_CACHE", "/tmp/dogeray_bench"), 709, 1920, 1080)
    sc = dr.Scene.load(path, "")
    sc.build_bvh()
    c = dr.Context(0)
    try:
        c.upload(sc)
        st = dr.pack_settings13(sc.settings(), 1)
        acc = _render(c, sc, st, 1920, 1080, 2)
        rgb, f = c.denoise(st, 1920, 1080, 2, out="both")
        a = c.render_aov(st, 1920, 1080, channels=("normal", "albedo", "depth", "material"))
    finally:
        c.close()
    want = hk.denoise(acc, st, 2, a["normal"], a["albedo"], a["depth"], a["material"], nthreads=8)
    _same((f, rgb), want, "C4 1920x1080")


@pytest.mark.parametrize("name", ["matball", "cube"])
def test_quality_after_four_frames(dr, ctx, synth, tmp_path, name):
    """256x256, 4 frames: the denoised image's MSE against a 4096-frame mean is at most half the raw mean's"""
    path = os.path.join(synth["dir"], "matball.rts") if name == "matball" else with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "c.rts"), CUBE_SETTINGS)
    sc = _load(dr, path)
    ctx.upload(sc)
    st = dr.pack_settings13(sc.settings(), 1)
    W, H = 256, 256
    ref = _render(ctx, sc, st, W, H, 4096, seed=1000).astype(np.float64).transpose(1, 0, 2) / 4096
    acc4 = _render(ctx, sc, st, W, H, 4, seed=77)
    raw = acc4.astype(np.float64).transpose(1, 0, 2) / 4
    den = ctx.denoise(st, W, H, 4, out="f32").astype(np.float64)
    mse_raw, mse_den = float(((raw - ref) ** 2).mean()), float(((den - ref) ** 2).mean())
    print("denoise quality %s: MSE raw %.3f denoised %.3f ratio %.3f" % (name, mse_raw, mse_den, mse_den / mse_raw))
    assert mse_den <= 0.5 * mse_raw, (mse_raw, mse_den)


def test_cache_ordering_and_what_it_leaves_alone(dr, hk, ctx, synth, tmp_path):
    path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube256.rts"), CUBE_SETTINGS)
    sc = _load(dr, path)
    ctx.upload(sc)
    s = sc.settings()
    st = dr.pack_settings13(s, 1)
    W, H = 256, 256
    ctx.accum_reset(W, H)
    # ordered behind dr_pipeline_submit: the call sees every frame submitted before it
    tickets = [ctx.pipeline_submit(st, W, H, s.background, 11 + 1000003 * k, present_divide_by=k + 1) for k in range(3)]
    got = ctx.denoise(st, W, H, 3, out="both")
    for t in tickets:
        ctx.pipeline_wait(t)
    acc = ctx.accum_read()
    _same(got[::-1], _host(hk, path, acc, st, 3), "behind the pipeline")
    # leaves the accumulator, the statistics and the options alone
    opts = {k: ctx.get_option(k) for k in ("kernel", "traversal", "pipe_group", "batch_frames", "denoise_tiles")}
    before = ctx.stats()
    ctx.denoise(st, W, H, 3)
    ctx.denoise(st, W, H, 3, out="f32", device=True)
    assert np.array_equal(ctx.accum_read(), acc) and ctx.stats() == before
    assert {k: ctx.get_option(k) for k in opts} == opts
    # the guide cache follows the view ...
    st2 = st.copy()
    st2[0] += 0.7
    st2[7] *= 1.1
    _same(ctx.denoise(st2, W, H, 3, out="both")[::-1], _host(hk, path, acc, st2, 3), "after a view change")
    _same(ctx.denoise(st, W, H, 3, out="both")[::-1], _host(hk, path, acc, st, 3), "back to the first view")
    # ... and the scene: another scene under the same settings
    other = with_settings(os.path.join(synth["dir"], "city_small.rts"), str(tmp_path / "city256.rts"), CUBE_SETTINGS)
    sc2 = _load(dr, other)
    ctx.upload(sc2)
    ctx.accum_reset(W, H)
    ctx.render_accumulate(st, W, H, s.background, 5, 1000003, 2)
    acc2 = ctx.accum_read()
    _same(ctx.denoise(st, W, H, 2, out="both")[::-1], _host(hk, other, acc2, st, 2), "after a scene upload")


def test_denoise_errors(dr, ctx, synth, tmp_path):
    st0 = np.zeros(13, np.float32) + 1
    empty = dr.Context(0)
    try:
        with pytest.raises(dr.DogerayError, match="no scene"):
            empty.denoise(st0, 64, 64, 1)
        path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "c.rts"), CUBE_SETTINGS)
        sc = _load(dr, path)
        empty.upload(sc)
        st = dr.pack_settings13(sc.settings(), 1)
        with pytest.raises(dr.DogerayError, match="accumulator"):
            empty.denoise(st, 256, 256, 1)
    finally:
        empty.close()
    ctx.upload(sc)
    ctx.accum_reset(256, 256)
    ctx.render_accumulate(st, 256, 256, sc.settings().background, 1, 1000003, 1)
    cases = [((st, 128, 256, 1), {}), ((st, 256, 255, 1), {}), ((st, 256, 256, 0), {}), ((st, 256, 256, -3), {}),
             ((st, 256, 256, 1), {"iterations": 11}), ((st, 256, 256, 1), {"iterations": -1}), ((st, 256, 256, 1), {"sigma_luminance": -1.0}),
             ((st, 256, 256, 1), {"sigma_depth": -0.01}), ((st, 256, 256, 1), {"normal_power_log2": 17})]
    bad = st.copy()
    bad[11] = 0
    cases.append(((bad, 256, 256, 1), {}))
    for args, params in cases:
        for device in (False, True):
            with pytest.raises(dr.DogerayError) as e:
                ctx.denoise(*args, device=device, **params)
            assert e.value.code == dr.ERR_INVALID, (args[1:], params)
    p = dr.denoise_params()
    rc = dr.lib().dr_accum_denoise(ctx._h, st.ctypes.data_as(C.c_void_p), 256, 256, 1, C.byref(p), None, None, 0)
    assert rc == dr.ERR_INVALID and "no output" in dr.lib().dr_last_error().decode()
    with pytest.raises(ValueError):
        ctx.denoise(st, 256, 256, 1, out="png")
    with pytest.raises(TypeError):
        ctx.denoise(st, 256, 256, 1, sigma=3)
    # a grid smaller than the accumulator and a 7-pixel-wide one: zeros outside the grid, nothing inside
    half = dr.pack_settings13(sc.settings(), 2)
    img = ctx.denoise(half, 256, 256, 1, out="f32")
    assert not img[128:].any() and not img[:, 128:].any() and img[:128, :128].any()


def test_cli_writes_the_denoised_image(dr, ctx, tmp_path):
    path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube.rts"), CUBE_SETTINGS)
    exe = os.path.join(ROOT, "dogeray_amd", "bin", "dogeray")
    out = str(tmp_path / "plain.ppm")
    pfm, ppm = str(tmp_path / "den.pfm"), str(tmp_path / "den.ppm")
    for target in (pfm, ppm):
        r = subprocess.run(["timeout", "-k", "10", "120", exe, path, "--frames", "1", "--quiet", "--out", out, "--denoise", target],
                           capture_output=True, text=True, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        assert "exported denoised image:" + target in r.stdout
    sc = _load(dr, path)
    ctx.set_traversal(2)
    ctx.upload(sc)
    pr = dr.ProgressiveRenderer(ctx, sc.settings())
    for _ in range(5):                       # the CLI's present loop: four preview steps and one frame, divide_by 2
        pr.step()
    rgb, f = ctx.denoise(pr.settings13(), pr.W, pr.H, 2, out="both")
    got = dr.read_pfm(pfm)
    assert got.shape == f.shape and dc.same_bits(got, f)
    data = open(ppm, "rb").read()
    assert data.startswith(b"P6\n%d %d\n255\n" % (pr.W, pr.H)) and np.array_equal(np.frombuffer(data[-pr.W * pr.H * 3:], np.uint8).reshape(rgb.shape), rgb)
    plain = open(out, "rb").read()
    assert np.array_equal(np.frombuffer(plain[-pr.W * pr.H * 3:], np.uint8).reshape(rgb.shape), pr.image(2))
