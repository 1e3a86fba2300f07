"""The camera rays' entry table on the GPU (option camera_entry).  Only the lean build and the counting build start camera rays at
their tile's entry and a single-frame launch of a view not seen before computes no table, so every context here forces the lean build
(coop_tiles_per_wave = 0) and launches two frames.  The device's table must equal the host build's (the same entry_leaf / entry_tile) word for word;
accumulators must be byte-identical with camera_entry 1 and 0, through both builds, with the same rays and fewer records."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import camera_entry_cases as cases
from camera_entry_cases import SEED, STRIDE

pytestmark = pytest.mark.gpu

W, H = 64, 40


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1
    return dogeray_amd


@pytest.fixture(scope="module")
def scenes(dr, synth, tmp_path_factory):
    """name -> the device's scene, its settings, settings13 at one sample per pixel and the host build's scene"""
    import host_kernel
    paths = cases.paths(synth, tmp_path_factory.mktemp("entrygpu"))
    out = {}
    for name in cases.NAMED + ("hf_0.02",):
        path, tex = paths[name]
        sc = dr.Scene.load(path, tex); sc.build_bvh()
        s = sc.settings()
        out[name] = {"path": path, "tex": tex, "scene": sc, "settings": s, "st": dr.pack_settings13(s, 1, spp=1), "host": host_kernel.Scene(path, tex)}
    return out


@pytest.fixture(scope="module")
def ctx(dr, scenes):          # scenes first: the generated scenes exist before this process touches the GPU
    c = dr.Context(0)
    c.set_option("coop_tiles_per_wave", 0)      # every launch runs the lean build (six waves per SIMD), or the counting build when counters are on
    yield c
    c.close()


def _build(ctx, count, tiles, frames):
    """the build the launch plan picks for such a launch (launch_plan.hpp plan_persistent on the host): a dict of its template arguments"""
    import host_kernel
    cfg = {"traversal": 2, "occupancy": ctx.get_option("occupancy"), "schedule": ctx.get_option("schedule"), "num_cus": 256,
           "coop_tiles_per_wave": ctx.get_option("coop_tiles_per_wave"), "count": int(count)}
    plan = host_kernel.persistent_plan(cfg, tiles * frames, ctx.get_option("coop_steps"), 0, 0)
    return dict(zip(host_kernel.BUILD_FIELDS, plan))


def _render(ctx, st, bg, frames=2, seed=SEED, counters=False, size=(W, H), **options):
    for k, v in options.items(): ctx.set_option(k, v)
    ctx.enable_counters(counters)
    ctx.stats_reset()
    ctx.accum_reset(*size)
    ctx.render_accumulate(st, size[0], size[1], bg, seed, STRIDE, frames)
    out = ctx.accum_read().copy()
    stats = ctx.stats()
    ctx.enable_counters(False)
    return out, stats


def _restore(ctx):
    ctx.set_option("camera_entry", 1); ctx.set_option("camera_cert", 1); ctx.set_option("cert_levels", 1)


@pytest.mark.parametrize("name", cases.NAMED)
def test_device_table_equals_the_host_builds(ctx, scenes, name):
    e = scenes[name]
    ctx.upload(e["scene"])
    assert ctx.get_option("traversal") == 2
    used = below = 0
    for st1 in cases.views(name, e["st"]):
        for k in range(3):
            st = cases.lens(st1, k)
            host = e["host"].camera_entry(st, W, H)
            _render(ctx, st, e["settings"].background, camera_entry=1)
            dev = ctx.camera_entry()
            if host is None:
                assert len(dev) == 0, (name, k)
                continue
            assert len(dev) == (W // 8) * (H // 8) and np.array_equal(dev, host[0]), (name, k, dev, host[0])
            used += 1
            below += int((dev != 0).sum())
    print("%s: %d tables equal the host's, %d tile words below the root or without geometry" % (name, used, below))
    assert used >= 2 and (below > 0 or not name.startswith("hf_"))      # (bunny_small's floor reaches behind the lens: every tile at the root, on both sides)
    _render(ctx, e["st"], e["settings"].background, camera_entry=0)
    assert len(ctx.camera_entry()) == 0
    _restore(ctx)


@pytest.mark.parametrize("count", [False, True])
@pytest.mark.parametrize("name", ["hf_0.1", "hf_0.02", "hf_1", "matball"])
def test_accumulators_do_not_depend_on_the_table(ctx, scenes, name, count):
    """through the lean build (count = False) and the counting build, with the certificate graded, single-step and off (hf_1 and matball have none)"""
    e = scenes[name]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    frames = 4
    b = _build(ctx, count, (W // 8) * (H // 8), frames)
    assert (b["count"], b["wide"], b["coop"]) == (int(count), 1, 0) and (count or b["occ"] == 6)      # the counting build, or the lean six-wave build
    for st in cases.views(name, e["st"]):
        for cert, levels in ((1, 1), (1, 0), (0, 1)):
            on, so = _render(ctx, st, bg, frames, counters=count, camera_entry=1, camera_cert=cert, cert_levels=levels)
            codes = ctx.camera_entry()
            assert len(codes) == (W // 8) * (H // 8)                                                    # the table was in use
            off, sf = _render(ctx, st, bg, frames, counters=count, camera_entry=0)
            assert len(ctx.camera_entry()) == 0
            assert np.array_equal(on, off), (name, cert, levels)
            assert so["frames"] == sf["frames"] == frames
            if count:
                assert so["rays"] == sf["rays"] and so["samples"] == sf["samples"]
                assert so["node_visits"] <= sf["node_visits"] and (so["node_visits"] < sf["node_visits"] or not name.startswith("hf_")), (name, cert, levels)
                print("%s cert %d levels %d: records per ray %.3f from the entries, %.3f from the root" %
                      (name, cert, levels, so["node_visits"] / so["rays"], sf["node_visits"] / sf["rays"]))
    _restore(ctx)


def test_frames_from_the_entries_equal_the_oracle(ctx, scenes):
    from oracle import orc
    for name in ("hf_0.1", "cube"):
        e = scenes[name]
        ctx.upload(e["scene"])
        bg = e["settings"].background
        st = cases.views(name, e["st"])[-1]
        got, _ = _render(ctx, st, bg, 2, camera_entry=1)
        assert (ctx.camera_entry() != 0).any()
        o = orc.Scene(e["path"], e["tex"] or None); o.build_bvh()
        want = sum(o.render(st, W, H, bg, SEED + STRIDE * k, nthreads=8)[0].astype(np.int64) for k in range(2))
        assert np.array_equal(got.astype(np.int64), want), name
    _restore(ctx)


def test_a_second_view_uses_its_own_table(ctx, scenes):
    e = scenes["hf_0.1"]
    ctx.upload(e["scene"])
    bg = e["settings"].background
    seen = set()
    for k in range(4):
        st = cases.top("hf_0.1", e["st"])
        st[0] += np.float32(0.07 * k); st[2] += np.float32(0.05 * k)          # the eye moves over the field: every launch a new view, right after the last
        on, _ = _render(ctx, st, bg, 2, seed=11 + k, camera_entry=1)
        dev = ctx.camera_entry()
        host = e["host"].camera_entry(st, W, H)
        assert host is not None and np.array_equal(dev, host[0]), k
        seen.add(dev.tobytes())
        off, _ = _render(ctx, st, bg, 2, seed=11 + k, camera_entry=0)
        assert np.array_equal(on, off), k
    assert len(seen) == 4
    # a stripe and a new scene drop the table as well
    ctx.set_stripe(2, 1)
    st = cases.top("hf_0.1", e["st"])
    on, _ = _render(ctx, st, bg, 2, size=(72, 44), camera_entry=1)
    host = e["host"].camera_entry(st, 72, 44, 2, 1)
    assert np.array_equal(ctx.camera_entry(), host[0])
    off, _ = _render(ctx, st, bg, 2, size=(72, 44), camera_entry=0)
    assert np.array_equal(on, off)
    ctx.set_stripe(1, 0)
    ctx.upload(scenes["hf_0.02"]["scene"])
    e2 = scenes["hf_0.02"]
    st2 = cases.top("hf_0.02", e2["st"])
    _render(ctx, st2, bg, 2, camera_entry=1)
    assert np.array_equal(ctx.camera_entry(), e2["host"].camera_entry(st2, W, H)[0])
    _restore(ctx)
