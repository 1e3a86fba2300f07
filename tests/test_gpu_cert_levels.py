"""The graded grazing certificate on the GPU (option cert_levels).  Only the lean build and the counting build carry it and a
single-frame launch of a view not seen before computes nothing, so every context here forces the lean build (coop_tiles_per_wave = 0).  The device's
grades must equal the host build's (the same cert_leaf) byte for byte; frames must be identical with cert_levels 1, cert_levels 0 and camera_cert 0
and equal the oracle's; the counting build must walk no more records with the grades than with the single step."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
from test_gpu_aov import _scaled_rts      # hf_small scaled down: its triangles enter the wide tree with their own bounds
import cert_level_cases as cases

pytestmark = pytest.mark.gpu

SEED, STRIDE = 5, 1000003


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1
    return dogeray_amd


@pytest.fixture(scope="module")
def scenes(dr, synth, tmp_path_factory):
    """per scale: path, dogeray scene, its settings, the host build's scene and the scene's own-bounds E"""
    import host_kernel
    out = {}
    d = tmp_path_factory.mktemp("certlevels")
    for scale in cases.SCALES:
        path = _scaled_rts(os.path.join(synth["dir"], "hf_small.rts"), str(d / ("hf_%g.rts" % scale)), scale)
        sc = dr.Scene.load(path, ""); sc.build_bvh()
        hs = host_kernel.Scene(path)
        own, mu = hs.wide_mu()
        out[scale] = {"path": path, "scene": sc, "settings": sc.settings(), "host": hs, "own": own, "e_own": float(mu[0])}
    return out


@pytest.fixture(scope="module")
def ctx(dr, scenes):          # scenes first: the generated scenes exist before this process touches the GPU
    c = dr.Context(0)
    c.set_option("coop_tiles_per_wave", 0)      # every launch runs the lean build (six waves per SIMD), the build that carries the certificate
    yield c
    c.set_option("cert_factor", 40); c.set_option("cert_levels", 1); c.set_option("camera_cert", 1)
    c.close()


_oracle = {}


def _reference(scenes, scale, name, W, H, frames):
    """the oracle's sum of `frames` frames of a view (computed once, shared)"""
    key = (scale, name, W, H, frames)
    if key not in _oracle:
        from oracle import orc
        e = scenes[scale]
        o = orc.Scene(e["path"], None); o.build_bvh()
        st = cases.view(_base(e), name, scale)
        _oracle[key] = sum(o.render(st, W, H, e["settings"].background, SEED + STRIDE * k, nthreads=8)[0].astype(np.int64) for k in range(frames))
        _oracle[key].setflags(write=False)
    return _oracle[key]


def _base(e):
    import dogeray_amd
    return dogeray_amd.pack_settings13(e["settings"], 1, spp=1)


def _upload(ctx, e):
    ctx.upload(e["scene"])
    assert ctx.get_option("wide_own_bounds") == e["own"] > 0


def _render(ctx, st, W, H, bg, frames, launches=1, seed=SEED, counters=False, **options):
    """`launches` launches of `frames` frames each of the same seeds (the last one is read): a one-frame launch of a new view computes no certificate,
    its second launch does"""
    for k, v in options.items(): ctx.set_option(k, v)
    ctx.enable_counters(counters)
    for _ in range(launches):
        ctx.stats_reset()
        ctx.accum_reset(W, H)
        ctx.render_accumulate(st, W, H, bg, seed, STRIDE, frames)
    out = ctx.accum_read().copy()
    stats = ctx.stats()
    ctx.enable_counters(False)
    return out, stats


@pytest.mark.parametrize("scale", cases.SCALES)
def test_device_grades_equal_the_host_builds(ctx, scenes, scale):
    e = scenes[scale]
    _upload(ctx, e)
    checked = graded = 0
    for W, H in cases.SIZES:
        for name in cases.VIEWS:
            st = cases.view(_base(e), name, scale)
            for factor in (1, 8, 40, 400):      # 1: a ladder clamped at the cut-off; 400: steps no tile of these views reaches
                for levels in (1, 0):
                    host = e["host"].cert_levels(st, W, H, factor, levels, e["e_own"])
                    _render(ctx, st, W, H, e["settings"].background, 2, cert_factor=factor, cert_levels=levels, camera_cert=1)
                    dev = ctx.cert_levels()
                    if host is None:
                        assert len(dev) == 0 and ctx.get_option("cert_flagged_permille") == -1
                        continue
                    plane, c = host
                    assert len(dev) == c["tiles"] == (W // 8) * (H // 8)
                    assert np.array_equal(dev, plane), (W, H, name, factor, levels, np.bincount(dev, minlength=6), c["tiles_per_grade"])
                    # the tile bits are "below the base step"
                    bits = np.unpackbits(ctx.cert_mask().view(np.uint8), bitorder="little")[:c["tiles"]].astype(bool)
                    assert np.array_equal(bits, dev <= c["base"]), (W, H, name, factor, levels)
                    checked += 1
                    graded += levels == 1 and len(set(dev.tolist()) - {0, 5}) > 0
    print("scale %g: %d planes equal the host's, %d of them with tiles between no step and every step" % (scale, checked, graded))
    assert checked >= 32
    if scale == 0.1: assert graded >= 4


@pytest.mark.parametrize("scale,size,name", [(0.1, (320, 192), "graze"), (0.1, (160, 96), "top"), (0.1, (320, 192), "scene"), (0.02, (160, 96), "graze")])
@pytest.mark.parametrize("frames", [1, 4])
def test_frames_do_not_depend_on_the_certificate(ctx, scenes, scale, size, name, frames):
    e = scenes[scale]
    _upload(ctx, e)
    W, H = size
    bg = e["settings"].background
    st = cases.view(_base(e), name, scale)
    want = _reference(scenes, scale, name, W, H, frames)
    launches = 2 if frames == 1 else 1
    graded, _ = _render(ctx, st, W, H, bg, frames, launches, cert_factor=40, cert_levels=1, camera_cert=1)
    assert len(ctx.cert_levels()) == (W // 8) * (H // 8)                  # the grades were in use
    flat, _ = _render(ctx, st, W, H, bg, frames, launches, cert_levels=0)
    assert set(ctx.cert_levels().tolist()) <= {0, 1}
    off, _ = _render(ctx, st, W, H, bg, frames, launches, camera_cert=0)
    assert len(ctx.cert_levels()) == 0
    assert np.array_equal(graded, flat) and np.array_equal(graded, off)
    assert np.array_equal(graded.astype(np.int64), want)
    ctx.set_option("camera_cert", 1); ctx.set_option("cert_levels", 1)


def test_counting_build_carries_the_grades(ctx, scenes):
    e = scenes[0.1]
    _upload(ctx, e)
    W, H = 320, 192
    bg = e["settings"].background
    for name in ("graze", "top"):
        st = cases.view(_base(e), name, 0.1)
        want = _reference(scenes, 0.1, name, W, H, 4)
        graded, sg = _render(ctx, st, W, H, bg, 4, counters=True, cert_factor=40, cert_levels=1, camera_cert=1)
        flat, sf = _render(ctx, st, W, H, bg, 4, counters=True, cert_levels=0)
        off, so = _render(ctx, st, W, H, bg, 4, counters=True, camera_cert=0)
        ctx.set_option("camera_cert", 1); ctx.set_option("cert_levels", 1)
        assert np.array_equal(graded.astype(np.int64), want) and np.array_equal(flat, graded) and np.array_equal(off, graded)
        assert sg["rays"] == sf["rays"] == so["rays"]
        print("%s: records per ray %.3f graded, %.3f single step, %.3f without a certificate" %
              (name, sg["node_visits"] / sg["rays"], sf["node_visits"] / sf["rays"], so["node_visits"] / so["rays"]))
        assert sg["node_visits"] <= sf["node_visits"] < so["node_visits"]


def test_moving_camera_recomputes_the_grades(ctx, scenes):
    e = scenes[0.1]
    _upload(ctx, e)
    W, H = 320, 192
    bg = e["settings"].background
    seen = set()
    for k in range(5):
        st = cases.view(_base(e), "graze", 0.1)
        st[1] = st[4] + np.float32(0.02 + 0.1 * k); st[0] += np.float32(0.03 * k)
        on, _ = _render(ctx, st, W, H, bg, 2, seed=11 + k, cert_factor=40, cert_levels=1, camera_cert=1)
        dev = ctx.cert_levels()
        host = e["host"].cert_levels(st, W, H, 40, 1, e["e_own"])
        assert host is not None and np.array_equal(dev, host[0]), k      # a launch of two frames computes the new view's grades
        seen.add(dev.tobytes())
        off, _ = _render(ctx, st, W, H, bg, 2, seed=11 + k, camera_cert=0)
        assert np.array_equal(on, off), k
    assert len(seen) == 5                                                 # a new view, new grades
    ctx.set_option("camera_cert", 1)


@pytest.mark.parametrize("scale", [0.2, 0.1, 0.02])
def test_fuzz_slice_levels_drawn_per_scene(dr, ctx, synth, tmp_path, scale):
    rng = np.random.default_rng(int(scale * 100) + 1)
    path = _scaled_rts(os.path.join(synth["dir"], "hf_small.rts"), str(tmp_path / "hf_scaled.rts"), scale)
    sc = dr.Scene.load(path, ""); sc.build_bvh()
    ctx.upload(sc)
    assert ctx.get_option("wide_own_bounds") > 0
    s = sc.settings()
    W, H = 160, 96
    used = 0
    for k in range(6):
        st = dr.pack_settings13(s, 1, spp=1)
        st[0:3] = st[3:6] + (st[0:3] - st[3:6]) * np.float32(rng.uniform(0.3, 1.5))
        st[1] = st[4] + np.float32(rng.uniform(0.05, 2.0) * scale)
        st[7] = np.float32(st[7] * rng.choice([1.0, 10.0]))              # |d| of a camera ray: the scene's focus distance or ten times it
        st[6] = np.float32(rng.choice([0.0, 0.01, 0.1]) * st[7])          # lens up to a tenth of the focus distance
        factor = int(rng.choice([1, 10, 40, 400]))
        levels = int(rng.integers(0, 2)) if k > 0 else 1
        a, _ = _render(ctx, st, W, H, s.background, 2, seed=100 + k, cert_factor=factor, cert_levels=levels, camera_cert=1)
        dev = ctx.cert_levels()
        if len(dev):
            assert dev.max() <= (5 if levels else 1), (scale, k)
            used += 1
        b, _ = _render(ctx, st, W, H, s.background, 2, seed=100 + k, camera_cert=0)
        assert np.array_equal(a, b), (scale, k, levels, factor)
    assert used >= 1
    ctx.set_option("cert_factor", 40); ctx.set_option("cert_levels", 1); ctx.set_option("camera_cert", 1)
