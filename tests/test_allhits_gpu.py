"""dr_trace_all_hits on the GPU (Context.trace_all) against the host build of the same functions (tools/host_kernel.cpp hk_allhits), bit for bit in
every channel: six scenes of tests/ray_cases.py, the ray counts around wave, workgroup and chunk edges, K in {0, 1, DR_ALLHITS_MAX}, both kernels
(the persistent one forced through option allhits_kernel), both trees; the device path on a torch side stream; channel subsets between guard
values; Context.contains and Context.nearest(signed=True) against the analytic answer on closed meshes; the refusals.
tests/test_allhits_host.py judges the host build against the brute-force definition without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES, CUBE_SETTINGS, with_settings
import ray_cases as rc
import ray_checks as ck

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu
F = np.float32
SURFACE = ("count", "t", "object", "material", "distance", "normal", "uv", "albedo")


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


_host_scenes = {}


def host_scene(hk, L):
    if L.stem not in _host_scenes:
        _host_scenes[L.stem] = hk.Scene(L.path)
    return _host_scenes[L.stem]


def upload(dr, ctx, path, wide_tree=2):
    ps = dr.Scene.load(path, "")
    ps.build_bvh()
    ctx.set_option("wide_tree", wide_tree)
    ctx.upload(ps)
    return ps


def differing(got, want):
    """channels of `want` whose bits differ in `got`"""
    out = []
    for k, w in want.items():
        g = np.asarray(got[k])
        same = np.array_equal(ck.bits(g), ck.bits(w)) if w.dtype == np.float32 else np.array_equal(g, w)
        if g.shape != w.shape or not same:
            out.append(k)
    return out


def second_hit_tmax(want):
    """a per-ray tmax that cuts the list in the middle or admits nothing: the t of the second listed hit, NaN, 0, or hit()'s own cap, in turn"""
    n = len(want["count"])
    second = np.where(want["count"] >= 2, want["t"][:, min(1, want["t"].shape[1] - 1)], F(10000)).astype(F)
    table = np.stack([second, np.full(n, np.nan, F), np.zeros(n, F), np.full(n, 10000, F)])
    return np.ascontiguousarray(table[np.arange(n) % 4, np.arange(n)])


@pytest.mark.parametrize("stem", ["tiny_2", "tiny_6", "ties", "grid_mixed", "cap", "degenerate"])
def test_trace_all_equals_the_host_build(dr, hk, ctx, tmp_path_factory, stem):
    L = ck.loaded(stem, tmp_path_factory)
    hs = host_scene(hk, L)
    KM = hk.allhits_max()
    assert KM == dr.ALLHITS_MAX
    assert hk.allhits_chunk() + 1 in rc.RAY_COUNTS      # one ray more than a chunk: the persistent kernel's second wave, its refill and its flush
    failed = []
    listed = 0
    try:
        for tree in (2, 1):
            upload(dr, ctx, L.path, tree)
            has_wide = ctx.get_option("wide_depth") > 0
            assert has_wide
            for n in rc.RAY_COUNTS:
                o, d = rc.mixed_rays(L.g, n)
                cut = second_hit_tmax(hs.allhits(o, d, None, KM, 3, 2, tree))
                for K in (0, 1, KM):
                    chan = SURFACE if K else ("count",)
                    for name, tmax in (("NULL", None), ("cut", cut)):
                        want = hs.allhits(o, d, tmax, K, 3, 2, tree, channels=chan)
                        listed += int((want["count"] > 0).sum())
                        for force in (1, 2):
                            ctx.set_option("allhits_kernel", force)
                            bad = differing(ctx.trace_all(o, d, tmax, K, channels=chan), want)
                            if bad:
                                failed.append("wide_tree %d, %d rays, K %d, tmax %s, kernel %d: %s" % (tree, n, K, name, force, ",".join(bad)))
            o, d = rc.mixed_rays(L.g, 257)
            for kinds, mask in ((("triangle",), 1), (("sphere",), 2)):
                want = hs.allhits(o, d, None, 3, mask, 2, tree)
                for force in (1, 2):
                    ctx.set_option("allhits_kernel", force)
                    if differing(ctx.trace_all(o, d, None, 3, kinds=kinds), want):
                        failed.append("wide_tree %d kinds %s kernel %d" % (tree, kinds, force))
    finally:
        ctx.set_option("allhits_kernel", 0)
        ctx.set_option("wide_tree", 2)
    assert listed > 0
    assert not failed, " | ".join(failed[:8])


def test_a_scene_without_a_wide_tree_walks_the_threaded_links(dr, hk, ctx, tmp_path_factory):
    L = ck.loaded("far_refused", tmp_path_factory)
    hs = host_scene(hk, L)
    upload(dr, ctx, L.path)
    assert ctx.get_option("wide_depth") == 0
    KM = hk.allhits_max()
    try:
        for force in (0, 2):                                      # (the persistent kernel cannot be forced where it does not exist)
            ctx.set_option("allhits_kernel", force)
            for n in (65, 1000):
                o, d = rc.mixed_rays(L.g, n)
                want = hs.allhits(o, d, None, KM, 3, 0, 1, channels=SURFACE)
                assert want["count"].max() >= 2
                assert not differing(ctx.trace_all(o, d, None, KM, channels=SURFACE), want)
    finally:
        ctx.set_option("allhits_kernel", 0)


def test_the_device_path_on_a_side_stream_equals_the_host_path(dr, hk, ctx, tmp_path_factory):
    import torch
    L = ck.loaded("grid_mixed", tmp_path_factory)
    upload(dr, ctx, L.path)
    dev = torch.device("cuda", 0)
    o, d = rc.mixed_rays(L.g, 1000)
    want = ctx.trace_all(o, d, None, 4, channels=SURFACE)
    assert want["count"].max() > 4
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        to, td = torch.from_numpy(o).to(dev, non_blocking=True), torch.from_numpy(d).to(dev, non_blocking=True)      # (the library's stream must wait for these)
        got = ctx.trace_all(to, td, None, 4, channels=SURFACE)
        host = {k: v.cpu().numpy() for k, v in got.items()}      # (and this stream for the library's)
    side.synchronize()
    assert all(v.device == dev for v in got.values())
    assert not differing(host, want)
    tm = torch.full((1000,), 0.5, dtype=torch.float32, device=dev)
    got = ctx.trace_all(to, td, tm, 0, channels=("count",))
    assert np.array_equal(got["count"].cpu().numpy(), ctx.trace_all(o, d, np.full(1000, 0.5, F), 0, channels=("count",))["count"])


GUARD = 64


def test_channel_subsets_write_nothing_else(dr, hk, ctx, tmp_path_factory):
    """dr_trace_all_hits with device pointers into the middle of buffers filled with a guard pattern: the words before and after every channel, and the
    whole buffer of a channel that was not asked for, keep the pattern"""
    import torch
    L = ck.loaded("grid_mixed", tmp_path_factory)
    hs = host_scene(hk, L)
    upload(dr, ctx, L.path)
    dev = torch.device("cuda", 0)
    n, K = 129, 3
    o, d = rc.mixed_rays(L.g, n)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    want = hs.allhits(o, d, None, K, 3, 2, 2, channels=SURFACE)
    words = {k: (n if dr.ALLHITS_CHANNELS[k][1] == 0 else n * K * dr.ALLHITS_CHANNELS[k][1]) for k in SURFACE}
    pattern = 0x5AA55AA5
    try:
        for force in (1, 2):
            ctx.set_option("allhits_kernel", force)
            for subset in (("count",), ("t",), ("object", "normal"), ("material",), SURFACE):
                buf = {k: torch.full((words[k] + 2 * GUARD,), pattern, dtype=torch.int32, device=dev) for k in SURFACE}
                torch.cuda.synchronize()
                rays, outs, params = dr.DrRayBuffers(), dr.DrAllHitsBuffers(), dr.DrAllHitsParams()
                rays.origin, rays.dir = to.data_ptr(), td.data_ptr()
                params.max_hits, params.kind_mask = K, 3
                for k in subset:
                    setattr(outs, k, buf[k].data_ptr() + 4 * GUARD)
                assert dr.lib().dr_trace_all_hits(ctx._h, n, C.byref(rays), C.byref(params), C.byref(outs), 1) == 0, dr.lib().dr_last_error()
                ctx.synchronize()
                for k in SURFACE:
                    a = buf[k].cpu().numpy()
                    if k not in subset:
                        assert (a == pattern).all(), "kernel %d, subset %s: channel %s was written" % (force, subset, k)
                        continue
                    assert (a[:GUARD] == pattern).all() and (a[-GUARD:] == pattern).all(), "kernel %d, subset %s: %s written out of bounds" % (force, subset, k)
                    body = a[GUARD:-GUARD].view(want[k].dtype).reshape(want[k].shape)
                    assert not differing({k: body}, {k: want[k]}), "kernel %d, subset %s: %s differs" % (force, subset, k)
    finally:
        ctx.set_option("allhits_kernel", 0)


# ------------------------------------------------------------------------------ contains, signed distances
def cube_boxes():
    """the eight axis-aligned cubes of tests/golden/scenes/cube.rts, twelve triangles each, found as the groups of triangles that share vertices:
    (lo, hi) [8, 3]"""
    groups = []      # sets of vertices
    for line in open(os.path.join(SCENES, "cube.rts")):
        f = line.strip().split(",")
        if len(f) >= 16 and not f[0].startswith("*"):
            tri = {tuple(float(x) for x in f[a:a + 3]) for a in (0, 9, 13)}
            touched = [g for g in groups if g & tri]
            groups = [g for g in groups if not (g & tri)] + [tri.union(*touched)]
    assert len(groups) == 8 and all(len(g) == 8 for g in groups)
    lo, hi = np.array([np.min(list(g), axis=0) for g in groups]), np.array([np.max(list(g), axis=0) for g in groups])
    assert np.allclose(hi - lo, 2.0, atol=1e-5)
    return lo, hi


def icosphere(levels):
    """a closed unit icosphere: vertices [v, 3] (on the unit sphere), triangles [f, 3]"""
    p = (1 + 5 ** 0.5) / 2
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [np.array(x) / np.linalg.norm(x) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2),
         (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, g = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v), np.array(f)


def check_contains(ctx, p, inside):
    import torch
    got = ctx.contains(p)
    assert got.dtype == bool and got.shape == (len(p),)
    wrong = np.nonzero(got != inside)[0]
    assert len(wrong) == 0, "%d of %d points wrong, first %r (inside: %s)" % (len(wrong), len(p), p[wrong[0]].tolist(), inside[wrong[0]])
    assert inside.sum() > len(p) // 20 and (~inside).sum() > len(p) // 20
    tp = torch.from_numpy(p).to(torch.device("cuda", 0))
    assert np.array_equal(ctx.contains(tp).cpu().numpy(), inside)
    unsigned, signed = ctx.nearest(p), ctx.nearest(p, signed=True)
    assert np.array_equal(ck.bits(np.abs(signed["distance"])), ck.bits(unsigned["distance"])) and np.array_equal(signed["object"], unsigned["object"])
    assert (unsigned["distance"] > 0).all() and np.array_equal(signed["distance"] < 0, inside)
    ts = ctx.nearest(tp, signed=True)["distance"].cpu().numpy()
    assert np.array_equal(ck.bits(ts), ck.bits(signed["distance"]))
    assert np.array_equal(ck.bits(ctx.nearest(p, signed=False)["distance"]), ck.bits(unsigned["distance"]))


def test_contains_on_the_cubes(dr, ctx, tmp_path):
    """cube.rts is eight closed cubes of side 2 that overlap: the parity rule says inside for a point in an odd number of them"""
    upload(dr, ctx, with_settings(os.path.join(SCENES, "cube.rts"), str(tmp_path / "cube.rts"), CUBE_SETTINGS))
    lo, hi = cube_boxes()
    rng = np.random.default_rng(31)
    p = rng.uniform(lo.min(axis=0) - 0.5, hi.max(axis=0) + 0.5, (6000, 3)).astype(F)
    pd = p.astype(np.float64)[:, None, :]
    off = np.minimum(np.abs(pd - lo[None]), np.abs(pd - hi[None])).min(axis=(1, 2))      # distance to the nearest face plane of any cube: >= 1e-2 of the side
    p = p[off >= 0.02]
    pd = p.astype(np.float64)[:, None, :]
    inside = ((pd > lo[None]) & (pd < hi[None])).all(axis=2).sum(axis=1) % 2 == 1
    assert len(p) > 3000
    check_contains(ctx, p, inside)


def test_contains_on_an_icosphere(dr, ctx, tmp_path):
    v, f = icosphere(2)
    centre, radius = np.array([0.3, -0.2, 0.5]), 1.5
    v = v * radius + centre
    path = rc._write(str(tmp_path / "icosphere.rts"), [rc.tri_line(v[a], v[b], v[c]) for a, b, c in f])
    upload(dr, ctx, path)
    # the polyhedron lies between its insphere and the sphere its vertices are on; float32 vertices move it by less than 1e-6
    tri = v[f].astype(F).astype(np.float64)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    inradius = np.abs(((tri[:, 0] - centre) * nrm).sum(axis=1)).min()
    rng = np.random.default_rng(32)
    p = (centre + rng.uniform(-1.3, 1.3, (6000, 3)) * radius).astype(F)
    r = np.linalg.norm(p.astype(np.float64) - centre, axis=1)
    keep = (r < inradius - 0.03) | (r > radius + 0.03)      # 1e-2 of the diameter away from the surface, on either side
    p, r = p[keep], r[keep]
    assert len(p) > 3000
    check_contains(ctx, p, r < inradius)


def test_errors_raise_before_a_launch(dr, ctx, tmp_path_factory):
    import torch
    L = ck.loaded("tiny_6", tmp_path_factory)
    upload(dr, ctx, L.path)
    o, d = rc.mixed_rays(L.g, 64)
    for kw in (dict(max_hits=-1), dict(max_hits=dr.ALLHITS_MAX + 1), dict(max_hits=0), dict(max_hits=0, channels=("count", "t")), dict(kinds=()),
               dict(kinds=("cone",)), dict(channels=()), dict(channels=("depth",))):
        with pytest.raises(ValueError):
            ctx.trace_all(o, d, **kw)
    to = torch.from_numpy(o).to(torch.device("cuda", 0))
    with pytest.raises(TypeError):
        ctx.trace_all(to, d)                                      # mixed numpy / torch
    with pytest.raises(TypeError):
        ctx.trace_all(to, to.double())
    with pytest.raises(ValueError):
        ctx.trace_all(to, to.cpu())
    for bad in ((o[:, :2], d), (o, d[:10]), (o.reshape(-1), d.reshape(-1))):
        with pytest.raises(ValueError):
            ctx.trace_all(*bad)
    with pytest.raises(ValueError):
        ctx.trace_all(o, d, np.zeros(3, F))
    with pytest.raises(ValueError):
        ctx.contains(o[:, :2])
    # the C entry itself
    rays, outs, params = dr.DrRayBuffers(), dr.DrAllHitsBuffers(), dr.DrAllHitsParams()
    cnt, t = np.zeros(64, np.int32), np.zeros((64, 4), F)
    rays.origin, rays.dir = o.ctypes.data, d.ctypes.data
    outs.count = cnt.ctypes.data
    call = lambda n=64, p=params: dr.lib().dr_trace_all_hits(ctx._h, n, C.byref(rays), C.byref(p), C.byref(outs), 0)
    for mh, km in ((-1, 3), (dr.ALLHITS_MAX + 1, 3), (4, 0), (4, 4)):
        params.max_hits, params.kind_mask = mh, km
        assert call() == dr.ERR_INVALID
    params.max_hits, params.kind_mask = 0, 3
    outs.t = t.ctypes.data
    assert call() == dr.ERR_INVALID                               # a K-shaped channel with K = 0
    outs.t = None
    assert call(-1) == dr.ERR_INVALID and call(1 << 31) == dr.ERR_INVALID
    assert call(0) == 0 and call() == 0
    rays.dir = None
    assert call() == dr.ERR_INVALID
    rays.dir = d.ctypes.data
    outs.count = None
    assert call() == dr.ERR_INVALID                               # no output channel
    assert ctx.trace_all(o[:0], d[:0])["t"].shape == (0, 4)
    fresh = dr.Context(0)
    try:
        with pytest.raises(dr.DogerayError) as e:
            fresh.trace_all(o, d)                                 # no scene
        assert e.value.code == dr.ERR_INVALID
    finally:
        fresh.close()


def test_bad_tensors_raise_with_the_messages_they_always_had(dr, ctx):
    """Context.trace_all through the shared marshaller (dogeray_amd._list_query): exception type and message, before anything is launched"""
    import torch
    dev = torch.device("cuda", 0)
    o = np.zeros((4, 3), F)
    to = torch.from_numpy(o).to(dev)
    cases = [
        (TypeError, "o, d and tmax must all be numpy arrays or all torch tensors", lambda: ctx.trace_all(to, o)),
        (ValueError, "d is on cpu, not on this context's cuda:0", lambda: ctx.trace_all(to, to.cpu())),
        (TypeError, "d must be float32, not torch.float64", lambda: ctx.trace_all(to, to.double())),
        (ValueError, "o must be contiguous", lambda: ctx.trace_all(to.t().contiguous().t(), to)),
        (ValueError, "o and d must both be [n, 3]", lambda: ctx.trace_all(to[:, :2].contiguous(), to)),
        (ValueError, "tmax must be [n]", lambda: ctx.trace_all(to, to, torch.ones(3, device=dev))),
    ]
    for kind, message, call in cases:
        with pytest.raises(kind) as e:
            call()
        assert type(e.value) is kind and str(e.value) == message
