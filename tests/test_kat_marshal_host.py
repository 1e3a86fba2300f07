"""The marshalling of the known-answer hooks (dogeray_amd.KAT_HOOKS, kat_marshal), without a GPU: every Context.kat_* wrapper and every host mirror
of tools/host_kernel.py judges the shapes of its arrays before it touches a library -- an input one row shorter than the first, or with a wrong
tail, is a ValueError that names hook and argument, where the library would have copied n rows out of the shorter array.  Then one well-formed
call of every host mirror against the same hk_kat_* function called through ctypes directly: the marshaller passes what the hand-written wrappers
passed."""
import ctypes as C

import numpy as np
import pytest

import shade_cases as sc
import shade_checks as ck

F, I, U32, U64 = np.float32, np.int32, np.uint32, np.uint64
N = 5

# hook -> its array arguments (name, dtype, shape tail) in the wrapper's order: the signatures, stated a second time
ARRAYS = {
    "rng": (),
    "aabb": (("o", F, (3,)), ("d", F, (3,)), ("mn", F, (3,)), ("mx", F, (3,))),
    "tri": (("o", F, (3,)), ("d", F, (3,)), ("v0", F, (3,)), ("v1", F, (3,)), ("v2", F, (3,))),
    "node_planes": (("w", U32, ()), ("a", F, ()), ("b", F, ())),
    "sphere": (("o", F, (3,)), ("d", F, (3,)), ("c", F, (3,)), ("r", F, ())),
    "optics": (("v", F, (3,)), ("nrm", F, (3,)), ("eta", F, ())),
    "normal": (("obj_index", I, ()), ("o", F, (3,)), ("d", F, (3,)), ("t", F, ())),
    "hit": (("o", F, (3,)), ("d", F, (3,))),
    "trace": (("o", F, (3,)), ("d", F, (3,))),
    "sample": (("seed", U64, ()), ("warm", I, ()), ("kind", I, ())),
    "outside": (("d2", F, ()),),
    "tex": (("tex", I, ()), ("u", F, ()), ("v", F, ())),
    "bounce": (("obj_index", I, ()), ("o", F, (3,)), ("d", F, (3,)), ("t", F, ()), ("atten", F, (3,)), ("seed", U64, ()), ("warm", I, ())),
    "miss": (("d", F, (3,)), ("atten", F, (3,))),
    "camera": (("x", I, ()), ("y", I, ()), ("sample", I, ())),
    "store": (("color", F, (3,)),),
    "tile_feedback": (("pixel_cost", U32, (64,)),),
    "order_split": (("order", I, ()), ("region_start", I, ()), ("key", U32, ())),
}
ST = np.array([0, 0, 2, 0, 0, 0, 0, 1, 45, 1, 1, 1, -1], F)
# how a wrapper f takes the arrays a beside its other arguments
CALL = {
    "miss": lambda f, a: f(*a, -1, 1.0),
    "camera": lambda f, a: f(ST, 64, 64, 0, 64, *a),
    "store": lambda f, a: f(*a, 1),
    "trace": lambda f, a: f(*a, 1),
}
HOST_FUNCTIONS = ("sample", "outside", "camera", "store")      # tools/host_kernel.py's, and the methods of its Scene:
HOST_METHODS = ("tex", "bounce", "miss")


class Touched(Exception):
    """a library was asked for"""


def touched():
    raise Touched()


def good(hook, n=N):
    return [np.zeros((n,) + tail, dt) for _, dt, tail in ARRAYS[hook]]


def bad_calls(hook):
    """(argument's name, the arrays with that argument misshapen): every input after the first one row short; every input with a tail one column wide;
    every input without one with a second axis of 2"""
    out = []
    for k, (name, dt, tail) in enumerate(ARRAYS[hook]):
        if k >= 1:
            a = good(hook)
            a[k] = a[k][:-1]
            out.append((name, a))
        a = good(hook)
        a[k] = np.zeros((N,) + (tail[:-1] + (tail[-1] + 1,) if tail else (2,)), dt)
        out.append((name, a))
    return out


def expect_refusals(hook, f):
    call = CALL.get(hook, lambda f, a: f(*a))
    for name, arrays in bad_calls(hook):
        with pytest.raises(ValueError) as e:
            call(f, arrays)
        tail = dict((nm, t) for nm, _, t in ARRAYS[hook])[name]
        assert str(e.value) == "kat_%s: %s must be [%s]" % (hook, name, ", ".join(["n"] + [str(k) for k in tail])), (hook, name)
    with pytest.raises(Touched):          # and arrays of the right shapes pass the checks: the call goes on to the library
        call(f, good(hook))


def test_the_table_states_the_signatures():
    import dogeray_amd as dr
    assert set(dr.KAT_HOOKS) == set(ARRAYS) and len(ARRAYS) == 18
    for hook, ins in ARRAYS.items():
        assert tuple((name, np.dtype(dt), tail) for name, dt, tail in dr.KAT_HOOKS[hook][0]) == tuple((name, np.dtype(dt), tail) for name, dt, tail in ins), hook


@pytest.mark.parametrize("hook", [h for h in ARRAYS if h not in ("rng", "tile_feedback", "order_split")])
def test_context_wrapper_judges_shapes_before_the_library(monkeypatch, hook):
    import dogeray_amd as dr
    monkeypatch.setattr(dr, "lib", touched)
    ctx = dr.Context.__new__(dr.Context)      # no device behind it: nothing below may reach one
    ctx._h = None
    assert len(bad_calls(hook)) >= 2 or len(ARRAYS[hook]) == 1
    expect_refusals(hook, getattr(ctx, "kat_" + hook))


def test_the_two_wrappers_with_a_count_of_their_own(monkeypatch):
    """kat_rng takes n as an argument and no array; kat_tile_feedback counts tiles -- ntiles, or the plane's size -- and keeps its own refusal"""
    import dogeray_amd as dr
    monkeypatch.setattr(dr, "lib", touched)
    ctx = dr.Context.__new__(dr.Context)
    ctx._h = None
    with pytest.raises(Touched):
        ctx.kat_rng(1, 4)
    pix = np.zeros(3 * 64 - 1, U32)
    with pytest.raises(ValueError) as e:
        ctx.kat_tile_feedback(pix, 1, 1, 400, 0, ntiles=3)          # one word short of three tiles
    assert str(e.value) == "pixel_cost holds fewer than ntiles * 64 words"
    with pytest.raises(Touched):
        ctx.kat_tile_feedback(pix, 1, 1, 400, 0)                    # its own count: two whole tiles
    with pytest.raises(Touched):
        ctx.kat_tile_feedback(pix.reshape(1, -1), 1, 1, 400, 0, ntiles=0)      # (the library refuses that one)


def test_the_order_split_wrapper_counts_its_key(monkeypatch):
    """kat_order_split counts tiles by its key; the order, if there is one, has as many entries, region_start at least regions + 1"""
    import dogeray_amd as dr
    monkeypatch.setattr(dr, "lib", touched)
    ctx = dr.Context.__new__(dr.Context)
    ctx._h = None
    rs = np.array([0, 2, 5], I)
    for kind, key in ((0, np.zeros(5, U32)), (1, np.ones(5, np.uint8))):
        with pytest.raises(ValueError) as e:
            ctx.kat_order_split(kind, 2, np.arange(4, dtype=I), rs, key)
        assert str(e.value) == "kat_order_split: order must be [n]"
        with pytest.raises(ValueError) as e:
            ctx.kat_order_split(kind, 3, None, rs, key)
        assert str(e.value) == "kat_order_split: region_start must hold regions + 1 entries"
        with pytest.raises(Touched):
            ctx.kat_order_split(kind, 2, None, rs, key)
        with pytest.raises(Touched):
            ctx.kat_order_split(kind, 2, np.arange(5, dtype=I)[::-1], rs, key)


@pytest.mark.parametrize("hook", HOST_FUNCTIONS + HOST_METHODS)
def test_host_mirror_judges_shapes_before_the_library(monkeypatch, hook):
    import host_kernel as hk
    monkeypatch.setattr(hk, "lib", touched)
    if hook in HOST_METHODS:
        owner = hk.Scene.__new__(hk.Scene)
        owner.h = None
    else:
        owner = hk
    expect_refusals(hook, getattr(owner, "kat_" + hook))


# ------------------------------------------------------------------ well-formed calls: the marshaller against ctypes by hand
def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def same(got, want):
    got = got if isinstance(got, tuple) else (got,)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes()


@pytest.fixture(scope="module")
def hk():
    import host_kernel
    host_kernel.build()
    return host_kernel


@pytest.fixture(scope="module")
def scene(hk, tmp_path_factory):
    return hk.Scene(*ck.files(tmp_path_factory))


def test_host_sample_outside_camera_store_pass_what_ctypes_passes(hk):
    L = hk.lib()
    n = 257
    i = np.arange(n, dtype=U64)
    seed, warm, kind = i * U64(sc.GOLDEN_RATIO) + U64(5), (i % U64(7)).astype(I), np.array(sc.SAMPLER_KINDS, I)[(i % U64(4)).astype(np.int64)]
    pt, nx = np.zeros((2, n, 3), F), np.zeros((2, n, 2), U32)
    assert L.hk_kat_sample(n, ptr(seed), ptr(warm), ptr(kind), ptr(pt[0]), ptr(nx[0]), ptr(pt[1]), ptr(nx[1])) == 0
    same(hk.kat_sample(seed, warm, kind), (pt, nx))
    assert np.abs(pt[:, kind == 3]).min(axis=2).max() > 0 and not pt[:, kind == 0].any()

    d2 = sc.outside_values()[(1 << 18) - 128:(1 << 18) + 129]
    out = np.zeros(len(d2), I)
    assert L.hk_kat_outside(len(d2), ptr(d2), ptr(out)) == 0
    same(hk.kat_outside(d2), (out,))
    assert out.min() == 0 and out.max() == 1

    st = sc.camera_views()["lens radius 0.3"]
    x, y, s = (a[:n].copy() for a in sc.camera_pixels(st))
    o, d, nxt = np.zeros((2, n, 3), F), np.zeros((2, n, 3), F), np.zeros((2, n, 2), U32)
    assert L.hk_kat_camera(ptr(st), sc.CAMERA_W, sc.CAMERA_H, 2 ** 32 + 7, 320, n, ptr(x), ptr(y), ptr(s), ptr(o), ptr(d), ptr(nxt)) == 0
    same(hk.kat_camera(st, sc.CAMERA_W, sc.CAMERA_H, 2 ** 32 + 7, 320, x, y, s), (o, d, nxt))
    assert np.abs(d).min(axis=2).max() > 0

    c = sc.store_colours()[:n]
    px = np.zeros((n, 3), I)
    assert L.hk_kat_store(n, ptr(c), 3, ptr(px)) == 0
    same(hk.kat_store(c, 3), (px,))
    assert (px != 0).any()


def test_host_scene_hooks_pass_what_ctypes_pass(hk, scene):
    L = hk.lib()
    tex, u, v = (a[::4001].copy() for a in sc.tex_cases())
    n = len(tex)
    rgba = np.zeros(n, U32)
    assert L.hk_kat_tex(scene.h, n, ptr(tex), ptr(u), ptr(v), ptr(rgba)) == 0
    same(scene.kat_tex(tex, u, v), (rgba,))
    assert n > 64 and len(np.unique(rgba)) > 8

    objs = sc.scene_objects()
    rng = np.random.default_rng(1)
    rays = [sc.object_rays(ob, rng, 4) for ob in objs]
    idx = np.repeat(np.arange(len(objs), dtype=I), 4)
    o, d, t = (np.ascontiguousarray(np.concatenate([r[k] for r in rays]), F) for k in range(3))
    n = len(idx)
    seed, warm = sc.bounce_seeds(n)
    atten = sc.bounce_attens(n)
    alive, nxt = np.zeros((2, n), I), np.zeros((2, n, 2), U32)
    o2, d2, a2 = (np.zeros((2, n, 3), F) for _ in range(3))
    assert L.hk_kat_bounce(scene.h, n, ptr(idx), ptr(o), ptr(d), ptr(t), ptr(atten), ptr(seed), ptr(warm), ptr(alive), ptr(o2), ptr(d2), ptr(a2), ptr(nxt)) == 0
    same(scene.kat_bounce(idx, o, d, t, atten, seed, warm), (alive, o2, d2, a2, nxt))
    assert n == 280 and alive.min() == 0 and alive.max() == 1

    dirs, att = (a[:257].copy() for a in sc.miss_directions())
    rgb = np.zeros((257, 3), F)
    assert L.hk_kat_miss(scene.h, 257, ptr(dirs), ptr(att), sc.TEX_ALBEDO, float(sc.MISS_BGINT), ptr(rgb)) == 0
    same(scene.kat_miss(dirs, att, sc.TEX_ALBEDO, sc.MISS_BGINT), (rgb,))
    assert (rgb > 0).any()
