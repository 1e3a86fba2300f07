"""The walks of dr_trace_rays compiled for the host (tools/host_kernel.cpp hk_trace = device_trace.hpp trace_threaded, trace_ordered, trace_wide;
hk_ray_surface = device_aov.hpp ray_surface) on every (scene, class) pair of tests/ray_cases.py, on the four walks of tests/test_rays_host.py:
closest hit with tmax NULL and with adversarial tmax values against the oracle's hit() filtered by t <= tmax, occlusion against the capped closest
walk and the same filter, and the surface pass against hk_aov.  No GPU: tests/test_gpu_trace.py compares the GPU with these functions bit for bit.

The contract (include/dogeray_amd.h "ray queries") is the filtered oracle for EVERY ray, so exact agreement is required on every pair -- also on the
pairs of class long_short and of the scenes far_mesh and far_refused, where the feature's issue would have let a walk that prunes its boxes against
tmax differ (a leaf whose computed box entry exceeds the t of its primitive: coordinates around 2^20).  Such a walk, measured before it was dropped from
this tree, differs on other pairs as well --
grid_mixed / graze 9 of 18000 rays, degenerate / axis 13, on_plane 8, inside 1, stadium / axis 6, on_plane 1, nonfinite 3 of 4000 each, with tmax on t
or one ulp above it: accepted hits whose float t lies in front of their own padded leaf box -- which is why the walks do not prune that way.

The feature's issue also asks for an assertion that the pairs outside its three excepted groups hold at least 80 % of the rays.  Counted from
ray_cases.PAIRS they hold 147000 of 186000, 79.03 %; with no pair excepted the assertion would say nothing, so there is none."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES, CUBE_SETTINGS, with_settings
import ray_cases as rc
import ray_checks as ck
import trace_cases as tc
from test_rays_host import WALKS, PAIRS

sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


_host_scenes = {}


def host_scene(hk, L):
    if L.stem not in _host_scenes:
        _host_scenes[L.stem] = hk.Scene(L.path)
    return _host_scenes[L.stem]


def differing(out, want_t, want_idx):
    return np.nonzero((ck.bits(out["t"]) != ck.bits(want_t)) | (out["object"] != want_idx))[0]


@pytest.mark.parametrize("stem,cls", PAIRS)
def test_tmax_null_returns_the_oracles_hits(hk, tmp_path_factory, stem, cls):
    L = ck.loaded(stem, tmp_path_factory)
    o, d, rt, ri = L.case(cls)
    hs = host_scene(hk, L)
    want_t, want_idx, want_occ = tc.post_filter(rt, ri, None)
    for traversal, tree in WALKS:
        out = hs.trace(o, d, None, traversal, tree)
        bad = differing(out, want_t, want_idx)
        assert len(bad) == 0, "%s / %s traversal %d wide_tree %d: %d of %d rays differ, first ray %d" % (stem, cls, traversal, tree, len(bad), len(o), bad[0])
        occ = hs.trace(o, d, None, traversal, tree, any_hit=True)["occluded"]
        assert np.array_equal(occ, want_occ), (stem, cls, traversal, tree)


@pytest.mark.parametrize("stem,cls", PAIRS)
def test_adversarial_tmax_is_the_filtered_oracle(hk, tmp_path_factory, stem, cls):
    L = ck.loaded(stem, tmp_path_factory)
    o, d, rt, ri = L.case(cls)
    hs = host_scene(hk, L)
    differ = []
    for name, tmax in tc.tmax_sets(stem, cls, rt):
        want_t, want_idx, want_occ = tc.post_filter(rt, ri, tmax)
        for traversal, tree in WALKS:
            out = hs.trace(o, d, tmax, traversal, tree)
            occ = hs.trace(o, d, tmax, traversal, tree, any_hit=True)["occluded"]
            # occlusion is the capped closest answer, on every pair: the host build against itself through two walks
            assert np.array_equal(occ, (out["t"] > 0).astype(np.int32)), (stem, cls, name, traversal, tree)
            assert np.array_equal(out["t"] > 0, out["object"] >= 0)
            bad = differing(out, want_t, want_idx)
            if len(bad) or not np.array_equal(occ, want_occ):
                differ.append("tmax %s traversal %d wide_tree %d: %d rays (first %d)" % (name, traversal, tree, len(bad), bad[0] if len(bad) else -1))
    assert not differ, "%s / %s differs from the filtered oracle -- %s" % (stem, cls, " | ".join(differ))


@pytest.mark.parametrize("stem", ["grid_mixed", "stadium"])
def test_tmax_lands_on_t_and_one_ulp_below(tmp_path_factory, stem):
    """of the rays the oracle hits (a miss has no t to land on): at least a quarter of the tmax values on the bits of t, a quarter one ulp below"""
    on = below = values = 0
    for cls, _ in rc.PAIRS[stem]:
        o, d, rt, ri = ck.loaded(stem, tmp_path_factory).case(cls)
        hit = rt > 0
        for name, tmax in tc.tmax_sets(stem, cls, rt):
            values += int(hit.sum())
            on += int((ck.bits(tmax)[hit] == ck.bits(rt)[hit]).sum())
            below += int((ck.bits(tmax)[hit] + 1 == ck.bits(rt)[hit]).sum())
    assert values > 0 and 4 * on >= values and 4 * below >= values, (on, below, values)


def test_any_hit_leaves_early(hk, tmp_path_factory):
    """the visit counter of the host build: the any-hit walk tests strictly fewer boxes than the closest walk over the `inside` and `axis` classes"""
    for traversal, tree in WALKS:
        closest = anyhit = 0
        for stem, cls in PAIRS:
            if cls not in ("inside", "axis"):
                continue
            L = ck.loaded(stem, tmp_path_factory)
            o, d, rt, ri = L.case(cls)
            hs = host_scene(hk, L)
            closest += int(hs.trace(o, d, None, traversal, tree, want_visits=True)["visits"].astype(np.int64).sum())
            anyhit += int(hs.trace(o, d, None, traversal, tree, any_hit=True, want_visits=True)["visits"].astype(np.int64).sum())
        print("traversal %d wide_tree %d: %d boxes tested by the closest walk, %d by the any-hit walk" % (traversal, tree, closest, anyhit))
        assert 0 < anyhit < closest, (traversal, tree)


def test_ray_counts_of_the_chunk_test_return_on_the_host(hk, tmp_path_factory):
    """the rays tests/test_gpu_trace.py sends through both kernels: the last one hits, so a dropped tail cannot pass for a miss"""
    L = ck.loaded("grid_mixed", tmp_path_factory)
    hs = host_scene(hk, L)
    for n in rc.RAY_COUNTS:
        o, d = rc.mixed_rays(L.g, n)
        rt, ri = L.orc.kat_hit(o, d)
        assert rt[-1] > 0
        want_t, want_idx, want_occ = tc.post_filter(rt, ri, None)
        for traversal, tree in WALKS:
            assert len(differing(hs.trace(o, d, None, traversal, tree), want_t, want_idx)) == 0, (n, traversal, tree)


SURFACE_SCENES = ("textest", "mats", "smooth")


def surface_scene(name, tmp_path):
    path = os.path.join(SCENES, name + ".rts")
    if not any(l.startswith("*") for l in open(path)):
        path = with_settings(path, str(tmp_path / (name + ".rts")), CUBE_SETTINGS)
    return path, (os.path.join(ROOT, "tests", "golden", "textures") if name == "textest" else "")


@pytest.mark.parametrize("name", SURFACE_SCENES)
def test_surface_pass_reproduces_the_aov_channels(hk, orc, tmp_path, name):
    """hk_aov's dir channel traced from the camera position: t, object, material, normal, uv, albedo and distance of hk_aov, bit for bit"""
    path, tex = surface_scene(name, tmp_path)
    o_ = orc.Scene(path, tex or None)
    o_.build_bvh()
    st = orc.settings13(o_.settings(), 1)
    W, H = 64, 48
    sc = hk.Scene(path, tex)
    a = sc.aov(st, W, H)
    n = a["t"].size
    assert a["t"].shape == (48, 64)
    d = np.ascontiguousarray(a["dir"].reshape(n, 3))
    origin = np.repeat(hk.camera_block(st, W, H)["from"][None], n, axis=0).astype(np.float32)
    channels = ("t", "object", "material", "normal", "uv", "albedo", "distance")
    for traversal, tree in ((2, 1), (0, 1), (1, 1)):      # (hk_aov walks the tree of wide_tree = 1)
        out = sc.trace(origin, d, None, traversal, tree, channels=channels)
        for k in channels:
            want = a[k].reshape(out[k].shape)
            same = np.array_equal(ck.bits(out[k]), ck.bits(want)) if want.dtype == np.float32 else np.array_equal(out[k], want)
            assert same, "%s channel %s traversal %d" % (name, k, traversal)
    assert (a["t"] > 0).any()


def test_context_trace_judges_numpy_shapes_without_a_gpu():
    """Context.trace's shape checks (the shared marshaller, dogeray_amd._list_query) raise before the library is called: type and message as ever"""
    import dogeray_amd as dr
    ctx = dr.Context.__new__(dr.Context)      # no device behind it: nothing below may reach one
    o = np.zeros((4, 3), np.float32)
    for bad in ((o, o[:3]), (o[:, :2], o), (o.reshape(-1), o.reshape(-1)), (None, o)):
        with pytest.raises(ValueError) as e:
            ctx.trace(*bad)
        assert str(e.value) == "o and d must both be [n, 3]"
    for kw in (dict(tmax=np.ones(3, np.float32)), dict(tmax=np.ones((4, 1), np.float32))):
        with pytest.raises(ValueError) as e:
            ctx.trace(o, o, **kw)
        assert str(e.value) == "tmax must be [n]"
