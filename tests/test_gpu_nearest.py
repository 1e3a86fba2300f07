"""dr_query_nearest on the GPU (Context.nearest) against the host build of the same functions (tools/host_kernel.cpp hk_nearest), bit for bit on every
channel: every (scene, class) pair of tests/nearest_cases.py over both trees with the rmax sets, the scene without a wide tree, the query counts
around wave and workgroup edges, the device path, channel subsets, the round trip with the ray query, the refusals.
tests/test_nearest_host.py judges the host build against the brute-force minimum and float64 without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES
import nearest_cases as nc
import ray_cases as rc

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
F = np.float32


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


_scenes = {}


def scene(hk, stem, tmp_path_factory):
    """(path, host scene, records) of a scene of the table, loaded once"""
    if stem not in _scenes:
        path = nc.write_scene(stem, str(tmp_path_factory.mktemp("gpu_nearest_" + stem)))
        hs = hk.Scene(path)
        _scenes[stem] = (path, hs, nc.Prims(hs.nearest_prims()))
    return _scenes[stem]


def upload(dr, ctx, path, wide_tree=2, tex=""):
    ps = dr.Scene.load(path, tex)
    ps.build_bvh()
    ctx.set_option("wide_tree", wide_tree)
    ctx.upload(ps)
    return ps


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def compare(failed, what, got, want, n):
    for k in want:
        if k == "visits":
            continue
        if not np.array_equal(bits(got[k]), bits(want[k])):
            bad = np.nonzero((bits(got[k]) != bits(want[k])).reshape(n, -1).any(axis=1))[0]
            failed.append("%s %s: %d of %d queries differ, first %d (GPU %r, host %r)" % (what, k, len(bad), n, bad[0], got[k][bad[0]].tolist(), want[k][bad[0]].tolist()))


@pytest.mark.parametrize("stem", nc.STEMS)
def test_nearest_equals_the_host_build(dr, hk, ctx, tmp_path_factory, stem):
    path, hs, g = scene(hk, stem, tmp_path_factory)
    channels = hk.NEAREST_CHANNELS
    failed = []
    try:
        for tree in (2, 1):
            upload(dr, ctx, path, tree)
            has_wide = ctx.get_option("wide_depth") > 0
            assert has_wide == (stem not in nc.NO_WIDE)
            if tree == 1 and not has_wide:
                continue                                          # (no wide tree: both uploads walk the same threaded links)
            for cls in nc.PAIRS[stem]:
                p = nc.points(stem, cls, g)
                want = hs.nearest(p, None, walk=2, tree=tree, nthreads=4)
                what = "%s / %s wide_tree %d" % (stem, cls, tree)
                compare(failed, what + " rmax NULL", ctx.nearest(p, channels=channels), want, len(p))
                if cls in ("near", "bad"):
                    for name, rmax in nc.rmax_sets(want["distance"]).items():
                        if rmax is not None and (tree == 2 or name == "mixed"):
                            compare(failed, what + " rmax " + name, ctx.nearest(p, rmax, channels=channels), hs.nearest(p, rmax, walk=2, tree=tree, nthreads=4), len(p))
    finally:
        ctx.set_option("wide_tree", 2)
    assert not failed, " | ".join(failed[:8])


def raw_nearest(dr, ctx, p, rmax, fields=("distance", "d2", "object", "material", "point", "uv")):
    """dr_query_nearest with device pointers into tensors preset to patterns no query returns (floats NaN, ints -7)"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(p)
    tp = torch.from_numpy(np.array(p)).to(dev)
    tr = torch.from_numpy(rmax).to(dev) if rmax is not None else None
    shape = {"point": (n, 3), "uv": (n, 2)}
    out = {k: (torch.full(shape.get(k, (n,)), -7, dtype=torch.int32, device=dev) if k in ("object", "material") else
               torch.full(shape.get(k, (n,)), float("nan"), dtype=torch.float32, device=dev)) for k in fields}
    torch.cuda.synchronize()
    pts, outs = dr.DrPointBuffers(), dr.DrNearestBuffers()
    pts.point, pts.rmax = tp.data_ptr(), (tr.data_ptr() if tr is not None else None)
    for k, a in out.items():
        setattr(outs, k, a.data_ptr())
    rc_ = dr.lib().dr_query_nearest(ctx._h, n, C.byref(pts), C.byref(outs), 1)
    assert rc_ == 0, dr.lib().dr_last_error()
    ctx.synchronize()
    return {k: a.cpu().numpy() for k, a in out.items()}


def test_query_counts_around_wave_and_workgroup_edges(dr, hk, ctx, tmp_path_factory):
    """n = 1 .. 1000 queries: the kernels' `i >= n`; the last point of every count lies on a surface, and a query no kernel wrote keeps its preset pattern"""
    path, hs, g = scene(hk, "grid_mixed", tmp_path_factory)
    upload(dr, ctx, path)
    failed = []
    for n in rc.RAY_COUNTS:
        p = nc.count_points(g, n)
        want = hs.nearest(p, walk=2, tree=2)
        assert want["object"][-1] >= 0 and want["distance"][-1] < 1e-3
        got = raw_nearest(dr, ctx, p, None)
        for k, a in got.items():
            assert not (np.isnan(a).any() if a.dtype == np.float32 else (a == -7).any()), "%d queries: %s left unwritten" % (n, k)
        compare(failed, "%d queries" % n, got, want, n)
    assert not failed, " | ".join(failed)


def test_device_path_equals_the_host_path_and_follows_torch_streams(dr, hk, ctx, tmp_path_factory):
    import torch
    path, hs, g = scene(hk, "grid_mixed", tmp_path_factory)
    upload(dr, ctx, path)
    p = nc.points("grid_mixed", "near", g)
    a = ctx.nearest(p, channels=hk.NEAREST_CHANNELS)
    rmax = nc.rmax_sets(a["distance"])["mixed"]
    dev = torch.device("cuda", 0)
    tp, tr = torch.from_numpy(p).to(dev), torch.from_numpy(rmax).to(dev)
    for cap_np, cap_t in ((None, None), (rmax, tr)):
        a, b = ctx.nearest(p, cap_np, channels=hk.NEAREST_CHANNELS), ctx.nearest(tp, cap_t, channels=hk.NEAREST_CHANNELS)
        for k in hk.NEAREST_CHANNELS:
            assert isinstance(b[k], torch.Tensor) and b[k].device == dev
            assert np.array_equal(bits(a[k]), bits(b[k].cpu().numpy())), k
    assert (a["object"] >= 0).any() and (a["object"] < 0).any()
    # on torch's current stream, no explicit synchronise: the points are made on a side stream right before the call, the result is consumed right
    # after it on the same stream
    free = ctx.nearest(p, channels=("distance",))["distance"]
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        moved = torch.from_numpy(p).to(dev).clone()                # (a kernel on the side stream writes the points the query reads)
        out = ctx.nearest(moved, channels=("distance",))["distance"]
        total = out.sum()
    side.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(free))
    assert float(total) == float(torch.from_numpy(free).to(dev).sum())


def test_a_channel_subset_equals_the_full_call(dr, hk, ctx, tmp_path_factory):
    path, hs, g = scene(hk, "ties", tmp_path_factory)
    upload(dr, ctx, path)
    p = nc.points("ties", "vertex_edge", g)
    full = ctx.nearest(p, channels=hk.NEAREST_CHANNELS)
    assert list(ctx.nearest(p)) == ["distance", "object"]
    for sub in (("distance",), ("d2",), ("object",), ("material",), ("point",), ("uv",), ("uv", "distance"), ("point", "material", "object")):
        got = ctx.nearest(p, channels=sub)
        assert list(got) == list(sub)
        for k in sub:
            assert np.array_equal(bits(got[k]), bits(full[k])), (sub, k)


def test_round_trip_with_the_ray_query(dr, hk, ctx):
    """points on Context.trace's hit positions o + t d of the camera rays of scene.rts: nearest returns a distance within the accuracy bound of 0, and
    the object the ray hit wherever the float64 brute force has a unique nearest object beyond that bound (at least half of the rays)"""
    path = os.path.join(SCENES, "scene.rts")
    ps = upload(dr, ctx, path)
    st = dr.pack_settings13(ps.settings(), 1)
    W, H = 96, 64
    a = ctx.render_aov(st, W, H, channels=("dir",))
    n = a["dir"].shape[0] * a["dir"].shape[1]
    d = np.ascontiguousarray(a["dir"].reshape(n, 3))
    o = np.repeat(hk.camera_block(st, W, H)["from"][None], n, axis=0).astype(F)
    tr = ctx.trace(o, d)
    hit = tr["t"] > 0
    assert hit.sum() > 1000
    p = (o[hit] + tr["t"][hit, None] * d[hit]).astype(F)
    hs = hk.Scene(path)
    g = nc.Prims(hs.nearest_prims())
    k = hk.nearest_k()
    # on the CPU first: the host build's answer on the same points meets the share
    host = hs.nearest(p)
    ratio, on_surface, share, differ, _ = nc.round_trip(g, p, tr["object"][hit], host["distance"], host["object"], k)
    assert ratio <= 1.0 and on_surface <= 1.0 and share >= 0.5 and differ == 0
    out = ctx.nearest(p)
    assert np.array_equal(bits(out["distance"]), bits(host["distance"])) and np.array_equal(out["object"], host["object"])
    ratio, on_surface, share, differ, brute_differ = nc.round_trip(g, p, tr["object"][hit], out["distance"], out["object"], k)
    print("round trip on scene.rts: %d rays, share compared %.3f, worst |distance - d64| / bound %.3f, worst d64 / bound at 0 %.3f" % (len(p), share, ratio, on_surface))
    assert (out["distance"].astype(np.float64) <= k * 2.0 ** -24 * 2 * g.lmax).all()
    assert ratio <= 1.0 and share >= 0.5 and differ == 0 and brute_differ == 0


def test_refusals(dr, hk, ctx, tmp_path_factory):
    import torch
    p = np.zeros((4, 3), F)

    def refused(call):
        with pytest.raises(dr.DogerayError) as e:
            call()
        assert e.value.code == dr.ERR_INVALID and len(str(e.value)) > 0
    empty = dr.Context(0)
    try:
        refused(lambda: empty.nearest(p))                         # no scene
    finally:
        empty.close()
    path, hs, g = scene(hk, "tiny_3", tmp_path_factory)
    upload(dr, ctx, path)
    want = hs.nearest(p)

    def raw(n, fields, point=True):
        f = np.full(4, np.nan, F)
        i = np.full(4, -7, np.int32)
        pts, outs = dr.DrPointBuffers(), dr.DrNearestBuffers()
        pts.point = p.ctypes.data if point else None
        for k in fields:
            setattr(outs, k, (i if k == "object" else f).ctypes.data)
        rc_ = dr.lib().dr_query_nearest(ctx._h, n, C.byref(pts), C.byref(outs), 0)
        return rc_, dr.lib().dr_last_error().decode(), f, i
    for n, fields, point in ((-1, ("distance",), True), (2 ** 31, ("distance",), True), (4, (), True), (4, ("distance", "object"), False)):
        rc_, msg, f, i = raw(n, fields, point)
        assert rc_ == dr.ERR_INVALID and msg, (n, fields, point)
        assert np.isnan(f).all() and (i == -7).all()              # nothing was launched, nothing written
        got = ctx.nearest(p)                                      # ... and the context answers the next valid call
        assert np.array_equal(bits(got["distance"]), bits(want["distance"])) and np.array_equal(got["object"], want["object"])
    rc_, msg, f, i = raw(0, ("distance",))
    assert rc_ == 0 and np.isnan(f).all()                         # n == 0: DR_OK, nothing launched
    assert ctx.nearest(np.zeros((0, 3), F))["distance"].shape == (0,)
    # Python: shapes, mixed kinds, devices, dtypes -- before anything is launched
    with pytest.raises(ValueError):
        ctx.nearest(p[:, :2])
    with pytest.raises(ValueError):
        ctx.nearest(p, rmax=np.ones(3, F))
    with pytest.raises(ValueError):
        ctx.nearest(p, channels=("distance", "normal"))
    with pytest.raises(ValueError):
        ctx.nearest(p, channels=())
    dev = torch.device("cuda", 0)
    tp = torch.from_numpy(p).to(dev)
    with pytest.raises(TypeError):
        ctx.nearest(tp, np.ones(4, F))                            # a tensor and an array
    with pytest.raises(ValueError):
        ctx.nearest(torch.from_numpy(p))                          # a tensor on the CPU
    with pytest.raises(TypeError):
        ctx.nearest(tp.double())
    with pytest.raises(TypeError):
        ctx.nearest(tp, torch.ones(4, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        ctx.nearest(torch.zeros((3, 4), dtype=torch.float32, device=dev).t())      # [4, 3], not contiguous
    got = ctx.nearest(tp)
    assert np.array_equal(bits(got["distance"].cpu().numpy()), bits(want["distance"])) and np.array_equal(got["object"].cpu().numpy(), want["object"])


def test_bad_tensors_raise_with_the_messages_they_always_had(dr, ctx):
    """Context.nearest through the shared marshaller (dogeray_amd._list_query): exception type and message, before anything is launched"""
    import torch
    dev = torch.device("cuda", 0)
    p = np.zeros((4, 3), F)
    tp = torch.from_numpy(p).to(dev)
    cases = [
        (TypeError, "p and rmax must both be numpy arrays or both torch tensors", lambda: ctx.nearest(tp, np.ones(4, F))),
        (ValueError, "p is on cpu, not on this context's cuda:0", lambda: ctx.nearest(torch.from_numpy(p))),
        (TypeError, "p must be float32, not torch.float64", lambda: ctx.nearest(tp.double())),
        (TypeError, "rmax must be float32, not torch.float64", lambda: ctx.nearest(tp, torch.ones(4, dtype=torch.float64, device=dev))),
        (ValueError, "p must be contiguous", lambda: ctx.nearest(torch.zeros((3, 4), dtype=torch.float32, device=dev).t())),
        (ValueError, "p must be [n, 3]", lambda: ctx.nearest(tp[:, :2].contiguous())),
        (ValueError, "rmax must be [n]", lambda: ctx.nearest(tp, torch.ones(3, device=dev))),
    ]
    for kind, message, call in cases:
        with pytest.raises(kind) as e:
            call()
        assert type(e.value) is kind and str(e.value) == message
