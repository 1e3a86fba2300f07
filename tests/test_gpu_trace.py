"""dr_trace_rays on the GPU (Context.trace) against the host build of the same functions (tools/host_kernel.cpp hk_trace, hk_ray_surface), bit for
bit: every (scene, class) pair of tests/ray_cases.py over both trees and every traversal, closest hit with tmax NULL and with the adversarial tmax
sets of tests/trace_cases.py, occlusion; the ray counts around the persistent kernel's chunk through both kernels; the scene without a wide tree;
the device path; the AOV round trip; the refusals.  tests/test_trace_host.py judges the host build against the oracle without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES, CUBE_SETTINGS, with_settings
import ray_cases as rc
import ray_checks as ck
import trace_cases as tc

sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu


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
def ctx(dr, synth):
    c = dr.Context(0)
    yield c
    c.close()


_host_scenes = {}


def host_scene(hk, L):
    if L.stem not in _host_scenes:
        _host_scenes[L.stem] = hk.Scene(L.path)
    return _host_scenes[L.stem]


def upload(dr, ctx, L, wide_tree=2):
    ps = dr.Scene.load(L.path, "")
    ps.build_bvh()
    ctx.set_option("wide_tree", wide_tree)
    ctx.upload(ps)
    return ps


def same(a, b):
    return np.array_equal(ck.bits(a), ck.bits(b)) if a.dtype == np.float32 else np.array_equal(a, b)


CHANNELS = ("t", "object", "material", "distance", "normal", "uv", "albedo")


def compare(failed, what, ctx, hs, o, d, tmax, traversal, tree, surface=False):
    """closest (t, object), occlusion and -- surface -- every channel of the rays on the GPU against the host build's"""
    got, want = ctx.trace(o, d, tmax), hs.trace(o, d, tmax, traversal, tree)
    for k in ("t", "object"):
        if not same(got[k], want[k]):
            bad = np.nonzero(ck.bits(got[k]) != ck.bits(want[k]) if k == "t" else got[k] != want[k])[0]
            failed.append("%s closest %s: %d of %d rays differ, first %d (GPU %r, host %r)" % (what, k, len(bad), len(o), bad[0], got[k][bad[0]], want[k][bad[0]]))
    occ, wocc = ctx.trace(o, d, tmax, any_hit=True)["occluded"], hs.trace(o, d, tmax, traversal, tree, any_hit=True)["occluded"]
    if not np.array_equal(occ, wocc):
        bad = np.nonzero(occ != wocc)[0]
        failed.append("%s occluded: %d of %d rays differ, first %d" % (what, len(bad), len(o), bad[0]))
    if surface:      # the surface pass on rays with origins of their own (and behind capped misses) against hk_ray_surface
        got, want = ctx.trace(o, d, tmax, channels=CHANNELS), hs.trace(o, d, tmax, traversal, tree, channels=CHANNELS)
        for k in CHANNELS:
            if not same(got[k], want[k]):
                g, w = got[k].reshape(len(o), -1), want[k].reshape(len(o), -1)
                bad = np.nonzero(((ck.bits(g) != ck.bits(w)) if g.dtype == np.float32 else (g != w)).any(axis=1))[0]
                failed.append("%s surface %s: %d of %d rays differ, first %d (GPU %r, host %r)" % (what, k, len(bad), len(o), bad[0], got[k][bad[0]], want[k][bad[0]]))


@pytest.mark.parametrize("stem", rc.STEMS)
def test_trace_equals_the_host_build(dr, hk, ctx, tmp_path_factory, stem):
    L = ck.loaded(stem, tmp_path_factory)
    hs = host_scene(hk, L)
    failed = []
    try:
        for tree in (2, 1):
            upload(dr, ctx, L, tree)
            has_wide = ctx.get_option("wide_depth") > 0
            if tree == 1 and not has_wide:
                continue                                          # (no wide tree: both uploads walk the same threaded links)
            traversals = (2, 0, 1) if tree == 2 and stem in ("grid_mixed", "ties", "tiny_3") else (2,)
            for traversal in traversals:
                ctx.set_traversal(traversal)
                # the wide walk through both kernels (so few rays would all go to the one-ray-per-lane kernel), the others through the only one they have
                for force in ((1, 2) if traversal == 2 and has_wide else (0,)):
                    ctx.set_option("trace_kernel", force)
                    for cls, _ in rc.PAIRS[stem]:
                        o, d, rt, ri = L.case(cls)
                        what = "%s / %s traversal %d wide_tree %d kernel %d" % (stem, cls, traversal, tree, force)
                        compare(failed, what + " tmax NULL", ctx, hs, o, d, None, traversal, tree, surface=True)
                        for name, tmax in tc.tmax_sets(stem, cls, rt):
                            compare(failed, what + " tmax " + name, ctx, hs, o, d, tmax, traversal, tree, surface=name == "mixed")
    finally:
        ctx.set_option("trace_kernel", 0)
        ctx.set_option("wide_tree", 2)
        ctx.set_traversal(dr.TRAVERSAL_WIDE)
    assert not failed, " | ".join(failed[:8])


def raw_trace(dr, ctx, mode, o, d, tmax):
    """dr_trace_rays with device pointers into tensors preset to patterns no walk returns (t NaN, object / occluded -7)"""
    import torch
    dev = torch.device("cuda", 0)
    n = len(o)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    tt = torch.from_numpy(tmax).to(dev) if tmax is not None else None
    t = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    obj = torch.full((n,), -7, dtype=torch.int32, device=dev)
    occ = torch.full((n,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rays, hits = dr.DrRayBuffers(), dr.DrHitBuffers()
    rays.origin, rays.dir, rays.tmax = to.data_ptr(), td.data_ptr(), (tt.data_ptr() if tt is not None else None)
    if mode == dr.TRACE_ANY:
        hits.occluded = occ.data_ptr()
    else:
        hits.t, hits.object = t.data_ptr(), obj.data_ptr()
    rc_ = dr.lib().dr_trace_rays(ctx._h, mode, n, C.byref(rays), C.byref(hits), 1)
    assert rc_ == 0, dr.lib().dr_last_error()
    ctx.synchronize()
    return t.cpu().numpy(), obj.cpu().numpy(), occ.cpu().numpy()


def test_ray_counts_around_the_chunk_through_both_kernels(dr, hk, ctx, tmp_path_factory):
    """n = 1 .. 1000 rays: the persistent kernel's 128-ray chunks and its `my < n && my < chunk_end` tail, the one-ray-per-lane kernel's `i >= n`; the
    last ray of every count hits, and a ray no kernel wrote keeps its preset pattern"""
    L = ck.loaded("grid_mixed", tmp_path_factory)
    hs = host_scene(hk, L)
    upload(dr, ctx, L)
    failed = []
    try:
        for n in rc.RAY_COUNTS:
            o, d = rc.mixed_rays(L.g, n)
            rt, ri = L.orc.kat_hit(o, d)
            assert rt[-1] > 0
            tmax = tc.tmax_sets("grid_mixed", "axis", rt)[3][1]
            for cap in (None, tmax):
                want = hs.trace(o, d, cap, 2, 2)
                wocc = hs.trace(o, d, cap, 2, 2, any_hit=True)["occluded"]
                if cap is None:
                    assert want["t"][-1] > 0 and wocc[-1] == 1
                for force in (1, 2):
                    ctx.set_option("trace_kernel", force)
                    t, obj, _ = raw_trace(dr, ctx, dr.TRACE_CLOSEST, o, d, cap)
                    _, _, occ = raw_trace(dr, ctx, dr.TRACE_ANY, o, d, cap)
                    assert not np.isnan(t).any() and (obj != -7).all() and (occ != -7).all(), "%d rays, kernel %d: rays left unwritten" % (n, force)
                    if not (same(t, want["t"]) and same(obj, want["object"]) and np.array_equal(occ, wocc)):
                        failed.append("%d rays, kernel %d, tmax %s" % (n, force, "NULL" if cap is None else "mixed"))
    finally:
        ctx.set_option("trace_kernel", 0)
    assert not failed, " | ".join(failed)


def test_a_scene_without_a_wide_tree_walks_the_threaded_links(dr, hk, ctx, tmp_path_factory):
    L = ck.loaded("far_refused", tmp_path_factory)
    hs = host_scene(hk, L)
    upload(dr, ctx, L)
    ctx.set_traversal(dr.TRAVERSAL_WIDE)
    assert ctx.get_option("wide_depth") == 0 and ctx.get_option("traversal") == 0
    failed = []
    try:
        for force in (0, 2):                                      # (the persistent kernel cannot be forced where it does not exist)
            ctx.set_option("trace_kernel", force)
            o, d, rt, ri = L.case("axis")
            assert (rt > 0).mean() > 0.05
            compare(failed, "far_refused / axis kernel %d" % force, ctx, hs, o, d, None, 2, 2)
    finally:
        ctx.set_option("trace_kernel", 0)
    assert not failed, " | ".join(failed)


@pytest.mark.parametrize("stem", ["tiny_2same", "tiny_2", "tiny_3", "tiny_4", "tiny_5", "tiny_6"])
def test_a_root_with_unused_child_slots(dr, hk, ctx, tmp_path_factory, stem):
    """both kernels over the smallest trees, both modes"""
    L = ck.loaded(stem, tmp_path_factory)
    hs = host_scene(hk, L)
    upload(dr, ctx, L)
    failed = []
    try:
        for force in (1, 2):
            ctx.set_option("trace_kernel", force)
            for cls, _ in rc.PAIRS[stem]:
                o, d, rt, ri = L.case(cls)
                compare(failed, "%s / %s kernel %d" % (stem, cls, force), ctx, hs, o, d, None, 2, 2)
                compare(failed, "%s / %s kernel %d tmax exact" % (stem, cls, force), ctx, hs, o, d, tc.tmax_sets(stem, cls, rt)[0][1], 2, 2)
    finally:
        ctx.set_option("trace_kernel", 0)
    assert not failed, " | ".join(failed)


def test_device_path_equals_the_host_path(dr, ctx, tmp_path_factory):
    import torch
    L = ck.loaded("grid_small", tmp_path_factory)
    upload(dr, ctx, L)
    o, d, rt, ri = L.case("graze")
    assert len(o) == 18000
    tmax = tc.tmax_sets("grid_small", "graze", rt)[3][1]
    dev = torch.device("cuda", 0)
    to, td, tt = (torch.from_numpy(np.array(a)).to(dev) for a in (o, d, tmax))      # (copies: the cases are read-only)
    for cap_np, cap_t in ((None, None), (tmax, tt)):
        a, b = ctx.trace(o, d, cap_np, channels=CHANNELS), ctx.trace(to, td, cap_t, channels=CHANNELS)
        for k in CHANNELS:
            assert isinstance(b[k], torch.Tensor) and b[k].device == dev
            assert same(a[k], b[k].cpu().numpy()), k
        occ_a, occ_b = ctx.trace(o, d, cap_np, any_hit=True), ctx.trace(to, td, cap_t, any_hit=True)
        assert list(occ_a) == ["occluded"] and np.array_equal(occ_a["occluded"], occ_b["occluded"].cpu().numpy())
    assert (a["t"] > 0).any() and (a["t"] < 0).any()


OPTIONS = ("kernel", "occupancy", "schedule", "heavy_factor", "coop_steps", "split_parts", "xcd_regions", "batch_frames", "feedback", "wide_tree", "moments",
           "camera_cert", "cert_factor", "cert_levels", "camera_entry", "sky_tiles", "trace_kernel", "traversal")


def test_a_trace_leaves_the_accumulator_the_statistics_and_the_options_alone(dr, ctx, tmp_path_factory):
    L = ck.loaded("grid_small", tmp_path_factory)
    ps = upload(dr, ctx, L)
    s = ps.settings()
    st = dr.pack_settings13(s, 1)
    W, H = 96, 64
    o, d, rt, ri = L.case("axis")

    def two_batches(trace):
        ctx.accum_reset(W, H)
        ctx.render_accumulate(st, W, H, s.background, 5, 1000003, 2)
        before = (ctx.accum_read().copy(), ctx.stats(), [ctx.get_option(k) for k in OPTIONS])
        if trace:
            ctx.trace(o, d, channels=CHANNELS)
            ctx.trace(o, d, any_hit=True)
            after = (ctx.accum_read().copy(), ctx.stats(), [ctx.get_option(k) for k in OPTIONS])
            assert np.array_equal(before[0], after[0]) and before[1] == after[1] and before[2] == after[2]
        ctx.render_accumulate(st, W, H, s.background, 5 + 2 * 1000003, 1000003, 2)
        return ctx.accum_read().copy()
    assert np.array_equal(two_batches(False), two_batches(True))

    def three_frames(trace):
        ctx.accum_reset(W, H)
        tickets = [ctx.pipeline_submit(st, W, H, s.background, 9 + k * 1000003) for k in range(3)]
        out = ctx.trace(o, d) if trace else None                  # right behind the submits, no wait
        acc = ctx.accum_read().copy()
        ctx.pipeline_wait(tickets[-1])
        return acc, out
    plain, _ = three_frames(False)
    traced, out = three_frames(True)
    assert plain.any() and np.array_equal(plain, traced)
    assert same(out["t"], ctx.trace(o, d)["t"])


def surface_scene(name, tmp_path):
    path = os.path.join(SCENES, name + ".rts")
    if not any(l.startswith("*") for l in open(path)):
        path = with_settings(path, str(tmp_path / (name + ".rts")), CUBE_SETTINGS)
    return path, (os.path.join(ROOT, "tests", "golden", "textures") if name == "textest" else "")


@pytest.mark.parametrize("name", ["textest", "smooth"])
def test_aov_round_trip(dr, hk, ctx, tmp_path, name):
    """render_aov's dir channel traced from the camera position reproduces render_aov's other channels bit for bit"""
    path, tex = surface_scene(name, tmp_path)
    ps = dr.Scene.load(path, tex)
    ps.build_bvh()
    ctx.set_option("wide_tree", 2)
    ctx.upload(ps)
    st = dr.pack_settings13(ps.settings(), 1)
    W, H = 64, 48
    a = ctx.render_aov(st, W, H)
    n = a["t"].size
    assert a["t"].shape == (48, 64) and (a["t"] > 0).any()
    d = np.ascontiguousarray(a["dir"].reshape(n, 3))
    origin = np.repeat(hk.camera_block(st, W, H)["from"][None], n, axis=0).astype(np.float32)
    try:
        for force in (1, 2):
            ctx.set_option("trace_kernel", force)
            out = ctx.trace(origin, d, channels=CHANNELS)
            for k in CHANNELS:
                assert same(out[k], a[k].reshape(out[k].shape)), "%s channel %s kernel %d" % (name, k, force)
    finally:
        ctx.set_option("trace_kernel", 0)


def test_refusals(dr, ctx, tmp_path_factory):
    import torch
    o = np.zeros((4, 3), np.float32)
    d = np.ones((4, 3), np.float32)

    def refused(call, code=None):
        with pytest.raises(dr.DogerayError) as e:
            call()
        assert e.value.code == (dr.ERR_INVALID if code is None else code) and len(str(e.value)) > 0
    empty = dr.Context(0)
    try:
        refused(lambda: empty.trace(o, d))                        # no scene
    finally:
        empty.close()
    L = ck.loaded("grid_small", tmp_path_factory)
    upload(dr, ctx, L)

    def raw(mode, n, fields, origin=True):
        t = np.full(4, np.nan, np.float32)
        i = np.full(4, -7, np.int32)
        rays, hits = dr.DrRayBuffers(), dr.DrHitBuffers()
        rays.origin, rays.dir = (o.ctypes.data if origin else None), d.ctypes.data
        for f in fields:
            setattr(hits, f, (t if f == "t" else i).ctypes.data)
        rc_ = dr.lib().dr_trace_rays(ctx._h, mode, n, C.byref(rays), C.byref(hits), 0)
        return rc_, dr.lib().dr_last_error().decode(), t, i
    for mode, n, fields, origin in ((0, -1, ("t",), True), (0, 2 ** 31, ("t",), True), (1, 4, ("occluded", "t"), True), (1, 4, ("occluded", "material"), True),
                                    (0, 4, ("t", "occluded"), True), (0, 4, (), True), (1, 4, (), True), (2, 4, ("t",), True), (-1, 4, ("t",), True),
                                    (0, 4, ("t",), False)):
        rc_, msg, t, i = raw(mode, n, fields, origin)
        assert rc_ == dr.ERR_INVALID and msg, (mode, n, fields)
        assert np.isnan(t).all() and (i == -7).all()              # nothing was launched, nothing written
    rc_, msg, t, i = raw(0, 0, ("t",))
    assert rc_ == 0 and np.isnan(t).all()                         # n == 0: DR_OK, nothing launched
    assert ctx.trace(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))["t"].shape == (0,)
    # Python: shapes, mixed kinds, devices, dtypes -- before anything is launched
    with pytest.raises(ValueError):
        ctx.trace(o, d[:3])
    with pytest.raises(ValueError):
        ctx.trace(o, d, tmax=np.ones(3, np.float32))
    with pytest.raises(ValueError):
        ctx.trace(o, d, channels=("t", "depth"))
    with pytest.raises(ValueError):
        ctx.trace(o, d, channels=("occluded",))
    dev = torch.device("cuda", 0)
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    with pytest.raises(TypeError):
        ctx.trace(to, d)                                          # a tensor and an array
    with pytest.raises(ValueError):
        ctx.trace(to, torch.from_numpy(d))                        # a tensor on the CPU
    with pytest.raises(TypeError):
        ctx.trace(to, td.double())
    with pytest.raises(ValueError):
        ctx.trace(to, td.t().contiguous().t())                    # not contiguous
    assert same(ctx.trace(to, td)["t"].cpu().numpy(), ctx.trace(o, d)["t"])


def test_probe_rays_are_the_rays_the_probe_walks(dr, ctx, synth):
    """dr_context_probe_rays (the measurement aid of tools/trace_rate.py): as many rays as dr_context_probe_trace reports for the same frame, camera rays
    first, no empty slot -- and they trace through the public path as through the host build"""
    path = os.path.join(synth["dir"], "city_small.rts")
    ps = dr.Scene.load(path, "")
    ps.build_bvh()
    ctx.set_option("wide_tree", 2)
    ctx.set_traversal(dr.TRAVERSAL_WIDE)
    ctx.upload(ps)
    s = ps.settings()
    st = dr.pack_settings13(s, 1, spp=1)
    W, H = 160, 96
    o, d = ctx.probe_rays(st, W, H, s.background, 7)
    rate, n, bad = ctx.probe_trace(st, W, H, s.background, 7, 1, 2)
    assert len(o) == len(d) == n and bad == 0 and n >= W // 8 * 8 * (H // 8 * 8)
    assert (d != 0).any(axis=1).all() and np.isfinite(o).all() and np.isfinite(d).all()
    t = ctx.trace(o, d)["t"]
    assert (t > 0).any() and (t < 0).any()


def test_bad_tensors_raise_with_the_messages_they_always_had(dr, ctx):
    """Context.trace through the shared marshaller (dogeray_amd._list_query): exception type and message, before anything is launched"""
    import torch
    dev = torch.device("cuda", 0)
    o = np.zeros((4, 3), np.float32)
    to = torch.from_numpy(o).to(dev)
    cases = [
        (TypeError, "o, d and tmax must all be numpy arrays or all torch tensors", lambda: ctx.trace(to, o)),
        (TypeError, "o, d and tmax must all be numpy arrays or all torch tensors", lambda: ctx.trace(o, o, tmax=torch.ones(4, device=dev))),
        (ValueError, "d is on cpu, not on this context's cuda:0", lambda: ctx.trace(to, torch.from_numpy(o))),
        (TypeError, "d must be float32, not torch.float64", lambda: ctx.trace(to, to.double())),
        (TypeError, "tmax must be float32, not torch.int32", lambda: ctx.trace(to, to, tmax=torch.ones(4, dtype=torch.int32, device=dev))),
        (ValueError, "d must be contiguous", lambda: ctx.trace(to, to.t().contiguous().t())),
        (ValueError, "o and d must both be [n, 3]", lambda: ctx.trace(to, to[:3])),
        (ValueError, "o and d must both be [n, 3]", lambda: ctx.trace(to.reshape(-1), to.reshape(-1))),
        (ValueError, "tmax must be [n]", lambda: ctx.trace(to, to, tmax=torch.ones(3, device=dev))),
    ]
    for kind, message, call in cases:
        with pytest.raises(kind) as e:
            call()
        assert type(e.value) is kind and str(e.value) == message
