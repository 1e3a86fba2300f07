"""First-hit AOV buffers on the GPU (dr_render_aov / Context.render_aov, pick, autofocus, dogeray --aov): bit for bit the host build of the same
device function, and the independent checks of tests/aov_checks.py (the oracle's kat_hit / kat_normal, numpy restatements) on the GPU's output."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import CUBE_SETTINGS, ROOT, SCENES, with_settings
import aov_checks

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


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


def _load(dr, orc, path, tex=""):
    sc = dr.Scene.load(path, tex)
    sc.build_bvh()
    o = orc.Scene(path, tex or None)
    o.build_bvh()
    return sc, o


def _same(a, b):
    if a.dtype == np.float32:
        return np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return np.array_equal(a, b)


def _scaled_rts(src, dst, k):
    """A copy of a scene of triangles with every position (vertices, camera, look-at, focus distance) times k"""
    out = []
    for line in open(src).read().split("\n"):
        c = line.split(",")
        if line.startswith("*"):
            for i in (1, 2, 3, 5, 6, 7, 8):
                c[i] = repr(float(c[i]) * k)
        elif len(c) > 15 and c[3].strip() == "2":
            for i in (0, 1, 2, 9, 10, 11, 13, 14, 15):
                c[i] = repr(float(c[i]) * k)
        out.append(",".join(c))
    open(dst, "w").write("\n".join(out))
    return dst


@pytest.mark.parametrize("mode", [2, 0, 1])
def test_gpu_aov_matches_the_host_build_and_the_oracle(dr, orc, hk, ctx, synth, tmp_path, mode):
    for name, path, tex, W, H in aov_checks.scene_cases(synth, tmp_path):
        sc, o = _load(dr, orc, path, tex)
        ctx.upload(sc)
        ctx.set_traversal(mode)
        st = dr.pack_settings13(sc.settings(), 1)
        got = ctx.render_aov(st, W, H)
        want = hk.Scene(path, tex).aov(st, W, H, traversal=mode)
        for k in aov_checks.CHANNELS:
            assert _same(got[k], want[k]), "%s traversal %d: channel %s differs from the host build" % (name, mode, k)
        aov_checks.check_against_oracle(got, o, st, W, H, (0, 0, W // 8 * 8, H // 8 * 8), "%s traversal %d" % (name, mode))
    ctx.set_traversal(2)


def test_own_bounds_tree_under_closest_hit_checks(dr, orc, ctx, synth, tmp_path):
    """hf_small at a tenth of its size with the focus distance at 1: its triangles enter the wide tree with their own bounds, and
    short camera rays must still find the oracle's closest hit"""
    path = _scaled_rts(os.path.join(synth["dir"], "hf_small.rts"), str(tmp_path / "hf10.rts"), 0.1)
    sc, o = _load(dr, orc, path)
    ctx.set_traversal(2)
    ctx.upload(sc)
    assert ctx.get_option("wide_own_bounds") > 0 and ctx.get_option("traversal") == 2
    st = dr.pack_settings13(sc.settings(), 1)
    st[7] = 1.0
    W, H = 320, 192
    a = ctx.render_aov(st, W, H, channels=("t", "object", "dir"))
    d = a["dir"].reshape(-1, 3)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 0.5
    t_ref, idx_ref = o.kat_hit(np.broadcast_to(st[0:3], d.shape), d)
    t, obj = a["t"].ravel(), a["object"].ravel()
    assert np.array_equal(t.view(np.uint32), t_ref.view(np.uint32))
    hit = t > 0
    assert hit.mean() > 0.2 and np.array_equal(obj[hit], idx_ref[hit]) and (obj[~hit] == -1).all()


def test_window_pick_autofocus(dr, orc, ctx, synth):
    path = os.path.join(synth["dir"], "city_small.rts")
    sc, o = _load(dr, orc, path)
    ctx.upload(sc)
    st = dr.pack_settings13(sc.settings(), 1)
    W, H = 160, 96
    full = ctx.render_aov(st, W, H)
    win = ctx.render_aov(st, W, H, window=(17, 9, 33, 21))
    for k in aov_checks.CHANNELS:
        assert _same(win[k], np.ascontiguousarray(full[k][9:30, 17:50])), k
    hit = np.argwhere(full["object"] >= 0)
    miss = np.argwhere(full["object"] < 0)
    for (y, x) in (tuple(hit[len(hit) // 2]), tuple(miss[0]) if len(miss) else tuple(hit[0]), (0, 0), (95, 159)):
        p = ctx.pick(st, W, H, int(x), int(y))
        for k in aov_checks.CHANNELS:
            v = full[k][y, x]
            assert _same(np.atleast_1d(np.asarray(p[k], dtype=v.dtype)), np.atleast_1d(v)), (k, x, y)
    af = ctx.autofocus(st, W, H)
    assert af.dtype == np.float32 and np.array_equal(np.delete(af, 7).view(np.uint32), np.delete(st, 7).view(np.uint32))
    assert full["object"][48, 80] >= 0 and af[7] == full["depth"][48, 80] and af[7] != st[7]
    assert np.array_equal(ctx.autofocus(st, W, H, int(hit[3][1]), int(hit[3][0]))[7:8], full["depth"][hit[3][0], hit[3][1]:hit[3][1] + 1])
    if len(miss):
        assert np.array_equal(ctx.autofocus(st, W, H, int(miss[0][1]), int(miss[0][0])).view(np.uint32), st.view(np.uint32))


def test_device_tensors_equal_host_buffers(dr, orc, ctx, synth):
    import torch
    path = os.path.join(synth["dir"], "hf_small.rts")
    sc, o = _load(dr, orc, path)
    ctx.upload(sc)
    st = dr.pack_settings13(sc.settings(), 1)
    host = ctx.render_aov(st, 320, 192)
    dev = ctx.render_aov(st, 320, 192, device=True)
    side = torch.zeros(1, device="cuda:0")
    for k in aov_checks.CHANNELS:
        assert dev[k].is_cuda and dev[k].device.index == 0
        side += dev[k].float().nan_to_num(posinf=0).sum() * 0      # consumed on torch's stream right away
        assert _same(dev[k].cpu().numpy(), host[k]), k
    sub = ctx.render_aov(st, 320, 192, window=(8, 16, 64, 40), channels=("depth", "normal"), device=True)
    assert set(sub) == {"depth", "normal"} and tuple(sub["normal"].shape) == (40, 64, 3)
    assert _same(sub["normal"].cpu().numpy(), np.ascontiguousarray(host["normal"][16:56, 8:72]))


def test_aov_between_pipelined_frames_changes_nothing(dr, orc, ctx, tmp_path):
    path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube256.rts"), CUBE_SETTINGS)
    sc, o = _load(dr, orc, path)
    ctx.upload(sc)
    s = sc.settings()
    st = dr.pack_settings13(s, 1)
    W, H = 256, 256
    seeds = [5 + 1000003 * k for k in range(4)]
    ref = [o.render(st, W, H, s.background, sd, nthreads=4)[0].astype(np.int64) for sd in seeds]
    ctx.accum_reset(W, H)
    tickets = [ctx.pipeline_submit(st, W, H, s.background, seeds[k], present_divide_by=k + 1) for k in range(3)]
    aov = ctx.render_aov(st, W, H, channels=("t", "object"))
    total = np.zeros((W, H, 3), np.int64)
    for k, t in enumerate(tickets):
        img = ctx.pipeline_wait(t, want_image=True)
        total += ref[k]
        assert np.array_equal(img, np.clip(total // (k + 1), 0, 255).astype(np.uint8).transpose(1, 0, 2)), "ticket %d" % k
    acc = ctx.accum_read()
    assert np.array_equal(acc.astype(np.int64), total)
    before = ctx.stats()
    ctx.render_aov(st, W, H)
    assert np.array_equal(ctx.accum_read(), acc) and ctx.stats() == before
    assert (aov["object"] >= 0).any()
    # a frame after an AOV call is the frame of a context that never made one
    frame = ctx.render_frame(st, W, H, s.background, seeds[3])
    fresh = dr.Context(0)
    try:
        fresh.upload(sc)
        assert np.array_equal(frame, fresh.render_frame(st, W, H, s.background, seeds[3]))
    finally:
        fresh.close()
    assert np.array_equal(frame.astype(np.int64), ref[3])


def test_aov_errors(dr, orc, ctx, tmp_path):
    empty = dr.Context(0)
    try:
        with pytest.raises(dr.DogerayError, match="no scene"):
            empty.render_aov(np.zeros(13, np.float32) + 1, 64, 64)
    finally:
        empty.close()
    path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "c.rts"), CUBE_SETTINGS)
    sc, o = _load(dr, orc, path)
    ctx.upload(sc)
    st = dr.pack_settings13(sc.settings(), 1)
    for window in ((0, 0, 0, 8), (0, 0, 8, 0), (250, 0, 8, 8), (0, -1, 8, 8), (0, 0, 257, 8)):
        with pytest.raises(dr.DogerayError) as e:
            ctx.render_aov(st, 256, 256, window=window)
        assert e.value.code == dr.ERR_INVALID and ("window" in str(e.value)), window
    # degenerate settings (test_degenerate_settings): accepted or refused as dr_render_frame does
    for line, W, H in (("*,7.358891,-6.925791,4.958309,0.01,0,0,0,3,45,0,1,1,no,100,70", 100, 70),
                       ("*,7.358891,-6.925791,4.958309,0.01,0,0,0,3,45,5,0,1,no,100,70", 100, 70),
                       ("*,7.358891,-6.925791,4.958309,0.01,0,0,0,3,45,3,2,1,no,37,23", 37, 23)):
        p = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "d.rts"), line)
        s2, _ = _load(dr, orc, p)
        ctx.upload(s2)
        st2 = dr.pack_settings13(s2.settings(), 2 if W == 37 else 1)
        ctx.render_frame(st2, W, H, s2.settings().background, 9)
        a = ctx.render_aov(st2, W, H)
        assert a["t"].shape == (dr.pixel_grid(st2, W, H)[1], dr.pixel_grid(st2, W, H)[0])
    bad = st.copy()
    bad[11] = 0
    for call in (lambda: ctx.render_frame(bad, 64, 64, 1.0, 1), lambda: ctx.render_aov(bad, 64, 64, window=(0, 0, 8, 8))):
        with pytest.raises(dr.DogerayError, match="divisor"):
            call()
    narrow = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "n.rts"), "*,7.358891,-6.925791,4.958309,0.01,0,0,0,3,45,3,1,1,no,7,200")
    s3, _ = _load(dr, orc, narrow)
    ctx.upload(s3)
    st3 = dr.pack_settings13(s3.settings(), 1)
    ctx.render_frame(st3, 7, 200, s3.settings().background, 9)          # nothing rendered, and nothing to see
    with pytest.raises(dr.DogerayError, match="window"):
        ctx.render_aov(st3, 7, 200)


def test_cli_writes_the_aovs(dr, orc, ctx, tmp_path):
    path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube.rts"), CUBE_SETTINGS)
    exe = os.path.join(ROOT, "dogeray_amd", "bin", "dogeray")
    prefix = str(tmp_path / "P")
    r = subprocess.run(["timeout", "-k", "10", "120", exe, path, "--frames", "1", "--quiet", "--aov", prefix], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    sc, o = _load(dr, orc, path)
    ctx.set_traversal(2)
    ctx.upload(sc)
    s = sc.settings()
    a = ctx.render_aov(dr.pack_settings13(s, 1), s.width, s.height)
    for k in ("depth", "distance", "normal", "albedo"):
        assert _same(dr.read_pfm(prefix + ".%s.pfm" % k), a[k]), k
    assert np.array_equal(dr.read_pfm(prefix + ".object.pfm"), a["object"].astype(np.float32))
    # --autofocus: the focus distance is the centre pixel's depth
    r2 = subprocess.run(["timeout", "-k", "10", "120", exe, path, "--frames", "1", "--quiet", "--autofocus"], capture_output=True, text=True, cwd=str(tmp_path))
    assert r2.returncode == 0, r2.stderr
    assert "autofocus: object %d" % a["object"][s.height // 2, s.width // 2] in r2.stdout


def test_full_size_c4_sampled_columns(dr, orc, tmp_path):
    """The 1M-triangle C4 stand-in at 1920x1080: t / object of every 24th column of the full AOV pass against the oracle"""
    sys.path.insert(0, ROOT)
    import bench
    path = bench.ensure_scene(os.environ.get("DOGERAY_BENCH_CACHE", "/tmp/dogeray_bench"), 709, 1920, 1080)
    sc = dr.Scene.load(path, "")
    sc.build_bvh()
    c = dr.Context(0)
    try:
        c.upload(sc)
        st = dr.pack_settings13(sc.settings(), 1)
        a = c.render_aov(st, 1920, 1080, channels=("t", "object", "dir"))
    finally:
        c.close()
    assert a["t"].shape == (1080, 1920)
    o = orc.Scene(path)
    o.build_bvh()
    cols = np.arange(5, 1920, 24)
    d = np.ascontiguousarray(a["dir"][:, cols]).reshape(-1, 3)
    t_ref, idx_ref = o.kat_hit(np.broadcast_to(st[0:3], d.shape), d)
    t, obj = np.ascontiguousarray(a["t"][:, cols]).ravel(), np.ascontiguousarray(a["object"][:, cols]).ravel()
    assert np.array_equal(t.view(np.uint32), t_ref.view(np.uint32))
    hit = t > 0
    assert 0.2 < hit.mean() < 1.0 and np.array_equal(obj[hit], idx_ref[hit]) and (obj[~hit] == -1).all()
    want = aov_checks.pinhole_dirs64(st, 1920, 1080, *np.meshgrid(cols, np.arange(1080)))
    assert (np.linalg.norm(d - want.reshape(-1, 3), axis=1) / np.linalg.norm(want.reshape(-1, 3), axis=1)).max() < 1e-6
