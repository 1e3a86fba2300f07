"""dr_trace_radiance on the GPU (Context.radiance) against the host build of the same function (tools/host_kernel.cpp hk_radiance), bit for bit:
every (scene, class) pair of tests/ray_cases.py over both trees, every traversal and both kernels; the all-materials scene of tests/shade_cases.py
with seeds and skips; the ray counts around the chunks and the waves; a frame of the renderer reproduced from its own camera rays; the device path; the
scene without a wide tree; the refusals.  tests/test_radiance_host.py judges the host build against the oracle without a GPU.

The comparison is tests/shade_checks.py's: bit patterns, and a NaN on one side asks for a NaN in the same place on the other (x86 and gfx950 form the
default NaN with different sign bits) -- the adversarial rays of tests/ray_cases.py (NaN and zero directions) produce them."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES, CUBE_SETTINGS, with_settings
import radiance_cases as rad
import ray_cases as rc
import ray_checks as rck
import shade_checks as ck

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

PLAIN, PERSISTENT = 1, 2          # option radiance_kernel


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
def ctx(dr):
    c = dr.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shading(dr, hk, tmp_path_factory):
    """the all-materials scene: (product scene, host scene, 4096 rays)"""
    rts, tex = ck.files(tmp_path_factory)
    ps = dr.Scene.load(rts, tex)
    ps.build_bvh()
    o, d = rad.shading_rays(4096 - rad.N_SKY, rad.N_SKY)
    return ps, hk.Scene(rts, tex), o, d


def restore(dr, ctx):
    ctx.set_option("radiance_kernel", 0)
    ctx.set_option("wide_tree", 2)
    ctx.set_traversal(dr.TRAVERSAL_WIDE)


def differ(got, want):
    """rays whose radiance or bounces differ"""
    return np.union1d(ck.differing(got["radiance"], want["radiance"]), ck.differing(got["bounces"], want["bounces"]))


BOTH = ("radiance", "bounces")
_host_scenes = {}


@pytest.mark.parametrize("stem", rc.STEMS)
def test_radiance_equals_the_host_build(dr, hk, ctx, tmp_path_factory, stem):
    """spp 1, max_depth 4 on every class of the scene, the adversarial ones among them: what the host build of the same function gives"""
    L = rck.loaded(stem, tmp_path_factory)
    if stem not in _host_scenes:
        _host_scenes[stem] = hk.Scene(L.path)
    hs = _host_scenes[stem]
    ps = dr.Scene.load(L.path, "")
    ps.build_bvh()
    failed, walked = [], 0
    try:
        for tree in (2, 1):
            ctx.set_option("wide_tree", tree)
            ctx.upload(ps)
            has_wide = ctx.get_option("wide_depth") > 0
            if tree == 1 and not has_wide:
                continue                                          # (no wide tree: both uploads walk the same threaded links)
            traversals = (2, 0, 1) if tree == 2 and stem in ("grid_mixed", "ties", "tiny_3") else (2,)
            for traversal in traversals:
                ctx.set_traversal(traversal)
                for cls, _ in rc.PAIRS[stem]:
                    o, d, rt, ri = L.case(cls)
                    want = hs.radiance(o, d, 1, 4, 1.0, -1, seed=7, traversal=traversal, tree=tree)
                    walked += int((want["bounces"] > 1).sum())
                    for force in ((PLAIN, PERSISTENT) if traversal == 2 and has_wide else (0,)):
                        ctx.set_option("radiance_kernel", force)
                        got = ctx.radiance(o, d, 1, 4, 1.0, -1, seed=7, channels=BOTH)
                        bad = differ(got, want)
                        if len(bad):
                            k = bad[0]
                            failed.append("%s / %s traversal %d wide_tree %d kernel %d: %d of %d rays differ, first %d (GPU %r %d, host %r %d)" % (
                                stem, cls, traversal, tree, force, len(bad), len(o), k, got["radiance"][k].tolist(), got["bounces"][k],
                                want["radiance"][k].tolist(), want["bounces"][k]))
    finally:
        restore(dr, ctx)
    assert not failed, " | ".join(failed[:8])
    assert walked > 0, "no ray of the scene bounces"


@pytest.mark.parametrize("backtex", rad.BACKGROUNDS, ids=["sky gradient", "backtex"])
def test_the_shading_scene_with_seeds_and_skips(dr, ctx, shading, backtex):
    """4096 rays, spp 3, max_depth 10, seeds and skip given, both kernels"""
    ps, hs, o, d = shading
    _, seeds, skip = rad.shading_seeds(len(o), True)
    want = hs.radiance(o, d, 3, 10, rad.BGINT, backtex, seeds=seeds, skip=skip)
    assert (want["bounces"] > 6).any() and np.isfinite(want["radiance"]).all()
    try:
        ctx.set_option("wide_tree", 2)
        ctx.upload(ps)
        for force in (PLAIN, PERSISTENT):
            ctx.set_option("radiance_kernel", force)
            got = ctx.radiance(o, d, 3, 10, rad.BGINT, backtex, seeds=seeds, skip=skip, channels=BOTH)
            ck.compare("GPU radiance kernel %d backtex %d" % (force, backtex), {"o": o, "d": d},
                       {"radiance": (got["radiance"], want["radiance"]), "bounces": (got["bounces"], want["bounces"])})
    finally:
        restore(dr, ctx)


def edge_counts(hk):
    """the counts around a wave, a workgroup and a chunk, and one with more chunks than the persistent grid has waves on any device up to 320 CUs"""
    waves = 320 * hk.radiance_occ() * 4
    return (1, 63, 64, 65, 127, 128, 129, 255, 257, 128 * (waves + 1) + 1)


def test_chunk_and_wave_edges_through_both_kernels(dr, hk, ctx, shading):
    """a dropped ray, a ray rendered twice, a stale cursor: n rays through both kernels equal the host build, and a call repeated behind a different
    call (which leaves other values in the context's staging) gives the same again"""
    ps, hs, o4, d4 = shading
    failed = []
    try:
        ctx.set_option("wide_tree", 2)
        ctx.upload(ps)
        for n in edge_counts(hk):
            reps = (n + len(o4) - 1) // len(o4)
            o, d = np.tile(o4, (reps, 1))[:n], np.tile(d4, (reps, 1))[:n]
            spp, depth = (2, 4) if n < 1000 else (1, 3)
            want = hs.radiance(o, d, spp, depth, rad.BGINT, -1, seed=n)
            for force in (PLAIN, PERSISTENT):
                ctx.set_option("radiance_kernel", force)
                first = ctx.radiance(o, d, spp, depth, rad.BGINT, -1, seed=n, channels=BOTH)
                ctx.radiance(o, d, spp, depth, rad.BGINT, -1, seed=n + 1, channels=BOTH)
                again = ctx.radiance(o, d, spp, depth, rad.BGINT, -1, seed=n, channels=BOTH)
                if len(differ(first, want)) or len(differ(again, want)):
                    failed.append("%d rays, kernel %d: %d differ from the host, %d in the repeated call" % (n, force, len(differ(first, want)), len(differ(again, want))))
    finally:
        restore(dr, ctx)
    assert not failed, " | ".join(failed)


@pytest.mark.parametrize("spp", [1, 2])
def test_a_frame_reproduced_from_its_own_camera_rays(dr, ctx, tmp_path, spp):
    """cube.rts at 64 x 64: every pixel's camera ray of every sample from Context.kat_camera, the generator's position behind it found in the
    oracle's sequence, sent through Context.radiance with the sample's seed and that skip; the samples summed in float on the host in sample
    order, stored by kat_store, equal the renderer's frame pixel for pixel.  spp 2 runs PER SAMPLE -- the samples of a pixel have camera rays of
    their own, so each is a call with spp = 1 and seeds = the full per-sample seed (sample term included)."""
    from oracle import orc
    path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube.rts"), CUBE_SETTINGS)
    ps = dr.Scene.load(path, "")
    ps.build_bvh()
    s = ps.settings()
    st = dr.pack_settings13(s, 1, spp=spp)
    W = H = 64
    frame_seed, stride = 4242, 8 * (W // 8)                       # (the seed stride of params_host.hpp: 8 * block columns)
    try:
        ctx.set_option("wide_tree", 2)
        ctx.upload(ps)
        frame = ctx.render_frame(st, W, H, s.background, frame_seed)
        assert frame.any()
        x, y = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(W), np.arange(H), indexing="ij"))
        pixel_seed = (np.uint64(frame_seed) + (x.astype(np.uint64) + y.astype(np.uint64) * np.uint64(stride)))
        for force in (PLAIN, PERSISTENT):
            ctx.set_option("radiance_kernel", force)
            colour = np.zeros((W * H, 3), np.float32)
            for k in range(spp):
                o, d, nx = ctx.kat_camera(st, W, H, frame_seed, stride, x, y, np.full(W * H, k, np.int32))
                seeds = pixel_seed + np.uint64((k * rad.GOLDEN_RATIO) % 2 ** 64)
                words = np.stack([orc.kat_rng_u32(int(v), 64) for v in seeds])
                m = (words[:, :-1] == nx[0][:, :1]) & (words[:, 1:] == nx[0][:, 1:])
                assert m.any(axis=1).all(), "a camera ray's draws were not found in the generator's first 64 outputs"
                skip = m.argmax(axis=1).astype(np.int32)
                got = ctx.radiance(o[0], d[0], 1, int(st[9]), s.background, int(st[12]), seeds=seeds, skip=skip)
                colour = colour + got["radiance"]
            stored = ctx.kat_store(colour, spp).reshape(W, H, 3)
            assert np.array_equal(stored, frame), "kernel %d: %d pixels differ from the frame" % (force, int((stored != frame).any(axis=2).sum()))
    finally:
        restore(dr, ctx)


OPTIONS = ("kernel", "occupancy", "schedule", "heavy_factor", "coop_steps", "split_parts", "xcd_regions", "batch_frames", "feedback", "wide_tree", "moments",
           "camera_cert", "cert_factor", "cert_levels", "camera_entry", "sky_tiles", "trace_kernel", "radiance_kernel", "traversal")


def test_device_path_and_a_call_between_submit_and_wait(dr, ctx, shading):
    """torch tensors in and out equal the host path; a call right behind pipeline_submit leaves the accumulator, the statistics and the options alone"""
    import torch
    ps, hs, o, d = shading
    _, seeds, skip = rad.shading_seeds(len(o), True)
    dev = torch.device("cuda", 0)
    try:
        ctx.set_option("wide_tree", 2)
        ctx.upload(ps)
        to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        ts, tk = torch.from_numpy(seeds.view(np.int64)).to(dev), torch.from_numpy(skip).to(dev)
        for force in (PLAIN, PERSISTENT):
            ctx.set_option("radiance_kernel", force)
            for kw_np, kw_t in (({}, {}), ({"seeds": seeds, "skip": skip}, {"seeds": ts, "skip": tk})):
                a = ctx.radiance(o, d, 2, 6, rad.BGINT, -1, seed=3, channels=BOTH, **kw_np)
                b = ctx.radiance(to, td, 2, 6, rad.BGINT, -1, seed=3, channels=BOTH, **kw_t)
                for k in BOTH:
                    assert isinstance(b[k], torch.Tensor) and b[k].device == dev
                    assert len(ck.differing(a[k], b[k].cpu().numpy())) == 0, (force, k)
        # a negative skip on the device path discards nothing, as 0
        zero = ctx.radiance(to, td, 1, 4, rad.BGINT, -1, seed=3, skip=torch.zeros_like(tk))["radiance"].cpu().numpy()
        neg = ctx.radiance(to, td, 1, 4, rad.BGINT, -1, seed=3, skip=torch.full_like(tk, -5))["radiance"].cpu().numpy()
        assert len(ck.differing(zero, neg)) == 0
        ctx.set_option("radiance_kernel", 0)
        s = ps.settings()
        st = dr.pack_settings13(s, 1, spp=1)
        W, H = 96, 64

        counted = ("frames", "launches", "samples", "rays", "node_visits", "prim_tests", "shades", "texels")      # (the others are timings)

        def three_frames(call):
            ctx.accum_reset(W, H)
            start = ctx.stats()
            tickets = [ctx.pipeline_submit(st, W, H, s.background, 9 + k * 1000003) for k in range(3)]
            out = ctx.radiance(o, d, 1, 6, rad.BGINT, -1, seed=3) if call else None          # right behind the submits, no wait
            acc = ctx.accum_read().copy()
            ctx.pipeline_wait(tickets[-1])
            end = ctx.stats()
            return acc, {k: end[k] - start[k] for k in counted}, [ctx.get_option(k) for k in OPTIONS], out
        plain, stats0, opts0, _ = three_frames(False)
        traced, stats1, opts1, out = three_frames(True)
        assert plain.any() and np.array_equal(plain, traced) and opts0 == opts1
        assert stats0 == stats1 and stats0["frames"] == 3, (stats0, stats1)
        before = (ctx.accum_read().copy(), ctx.stats())
        again = ctx.radiance(o, d, 1, 6, rad.BGINT, -1, seed=3)
        assert np.array_equal(before[0], ctx.accum_read()) and before[1] == ctx.stats()
        assert len(ck.differing(out["radiance"], again["radiance"])) == 0
    finally:
        restore(dr, ctx)


def test_a_scene_without_a_wide_tree_walks_the_threaded_links(dr, hk, ctx, tmp_path_factory):
    L = rck.loaded("far_refused", tmp_path_factory)
    hs = hk.Scene(L.path)
    ps = dr.Scene.load(L.path, "")
    ps.build_bvh()
    try:
        ctx.set_option("wide_tree", 2)
        ctx.upload(ps)
        ctx.set_traversal(dr.TRAVERSAL_WIDE)
        assert ctx.get_option("wide_depth") == 0 and ctx.get_option("traversal") == 0
        o, d, rt, ri = L.case("axis")
        assert (rt > 0).mean() > 0.05
        want = hs.radiance(o, d, 2, 4, 1.0, -1, seed=11, traversal=2, tree=2)
        for force in (0, PERSISTENT):                             # (the persistent kernel cannot be forced where it does not exist)
            ctx.set_option("radiance_kernel", force)
            assert len(differ(ctx.radiance(o, d, 2, 4, 1.0, -1, seed=11, channels=BOTH), want)) == 0, force
    finally:
        restore(dr, ctx)


def test_panorama_tool(dr, ctx, tmp_path):
    """tools/panorama.py on cube.rts: the zenith row sees the sky gradient's blue end, the image is finite and survives the .pfm"""
    import panorama
    path = with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube.rts"), CUBE_SETTINGS)
    ps = dr.Scene.load(path, "")
    ps.build_bvh()
    try:
        ctx.set_option("wide_tree", 2)
        ctx.upload(ps)
        s = ps.settings()
        img = panorama.render(ctx, s, 64, 2)
        assert img.shape == (32, 64, 3) and img.dtype == np.float32 and np.isfinite(img).all() and img.any()
        # straight up the gradient is (0.5, 0.7, 1.0) x background, straight down (were it not for the scene) white: the top row is bluer than red
        top = img[0].mean(axis=0)
        assert top[2] > top[0] and abs(top[2] - s.background) < 0.05 * s.background, top
        assert np.array_equal(dr.read_pfm(dr.write_pfm(str(tmp_path / "pano.pfm"), img)), img)
    finally:
        restore(dr, ctx)


def test_refusals(dr, ctx, shading):
    import torch
    ps, hs, o, d = shading
    o, d = np.ascontiguousarray(o[:4]), np.ascontiguousarray(d[:4])

    def refused(call):
        with pytest.raises(dr.DogerayError) as e:
            call()
        assert e.value.code == dr.ERR_INVALID and len(str(e.value)) > 0
    empty = dr.Context(0)
    try:
        refused(lambda: empty.radiance(o, d))                     # no scene
    finally:
        empty.close()
    ctx.set_option("wide_tree", 2)
    ctx.upload(ps)

    def raw(n, spp=1, max_depth=4, backtex=-1, origin=True, dirs=True, radiance=True, bounces=False, skip=None):
        r = np.full((4, 3), np.nan, np.float32)
        b = np.full(4, -7, np.int32)
        rays, params, out = dr.DrRadianceRays(), dr.DrRadianceParams(), dr.DrRadianceOut()
        assert dr.lib().dr_radiance_defaults(C.byref(params)) == 0
        params.spp, params.max_depth, params.backtex = spp, max_depth, backtex
        rays.origin, rays.dir = (o.ctypes.data if origin else None), (d.ctypes.data if dirs else None)
        rays.skip = skip.ctypes.data if skip is not None else None
        out.radiance, out.bounces = (r.ctypes.data if radiance else None), (b.ctypes.data if bounces else None)
        rc_ = dr.lib().dr_trace_radiance(ctx._h, n, C.byref(rays), C.byref(params), C.byref(out), 0)
        return rc_, dr.lib().dr_last_error().decode(), r, b
    n_tex = len(rad.sc.TEXTURES)
    for kw in ({"n": -1}, {"n": 2 ** 31}, {"n": 4, "origin": False}, {"n": 4, "dirs": False}, {"n": 4, "radiance": False}, {"n": 4, "spp": 0},
               {"n": 4, "max_depth": 0}, {"n": 4, "backtex": n_tex}, {"n": 4, "skip": np.array([0, 2, -1, 0], np.int32)}):
        rc_, msg, r, b = raw(**kw)
        assert rc_ == dr.ERR_INVALID and msg, kw
        assert np.isnan(r).all() and (b == -7).all()              # nothing was launched, nothing written
    rc_, msg, r, b = raw(0)
    assert rc_ == 0 and np.isnan(r).all()                         # n == 0: DR_OK, nothing launched
    rc_, msg, r, b = raw(4, backtex=n_tex - 1, bounces=True, skip=np.array([0, 2, 1, 0], np.int32))
    assert rc_ == 0 and np.isfinite(r).all() and (b >= 1).all()
    assert ctx.radiance(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))["radiance"].shape == (0, 3)
    # Python: shapes, channels, mixed kinds, devices, dtypes -- before anything is launched
    with pytest.raises(ValueError):
        ctx.radiance(o, d[:3])
    with pytest.raises(ValueError):
        ctx.radiance(o, d, seeds=np.zeros(3, np.uint64))
    with pytest.raises(ValueError):
        ctx.radiance(o, d, channels=("radiance", "t"))
    with pytest.raises(ValueError):
        ctx.radiance(o, d, channels=())
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    with pytest.raises(TypeError):
        ctx.radiance(to, d)                                       # a tensor and an array
    with pytest.raises(ValueError):
        ctx.radiance(to, torch.from_numpy(d))                     # a tensor on the CPU
    with pytest.raises(TypeError):
        ctx.radiance(to, td.double())
    with pytest.raises(TypeError):
        ctx.radiance(to, td, skip=torch.zeros(4, dtype=torch.int64, device=dev))
    restore(dr, ctx)


def test_bad_tensors_raise_with_the_messages_they_always_had(dr, ctx):
    """Context.radiance through the shared marshaller (dogeray_amd._list_query): exception type and message, before anything is launched"""
    import torch
    dev = torch.device("cuda", 0)
    o = np.zeros((4, 3), np.float32)
    to = torch.from_numpy(o).to(dev)
    cases = [
        (TypeError, "o, d, seeds and skip must all be numpy arrays or all torch tensors", lambda: ctx.radiance(to, o)),
        (TypeError, "o, d, seeds and skip must all be numpy arrays or all torch tensors", lambda: ctx.radiance(to, to, skip=np.zeros(4, np.int32))),
        (ValueError, "d is on cpu, not on this context's cuda:0", lambda: ctx.radiance(to, torch.from_numpy(o))),
        (TypeError, "d must be torch.float32, not torch.float64", lambda: ctx.radiance(to, to.double())),
        (TypeError, "seeds must be torch.int64, not torch.int32", lambda: ctx.radiance(to, to, seeds=torch.zeros(4, dtype=torch.int32, device=dev))),
        (TypeError, "skip must be torch.int32, not torch.int64", lambda: ctx.radiance(to, to, skip=torch.zeros(4, dtype=torch.int64, device=dev))),
        (ValueError, "d must be contiguous", lambda: ctx.radiance(to, to.t().contiguous().t())),
        (ValueError, "o and d must both be [n, 3]", lambda: ctx.radiance(to, to[:3])),
        (ValueError, "seeds and skip must be [n]", lambda: ctx.radiance(to, to, seeds=torch.zeros(3, dtype=torch.int64, device=dev))),
    ]
    for kind, message, call in cases:
        with pytest.raises(kind) as e:
            call()
        assert type(e.value) is kind and str(e.value) == message
