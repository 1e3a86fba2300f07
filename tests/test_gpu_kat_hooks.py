"""The staging of the known-answer hooks on the GPU (dogeray_amd/csrc/context_probe.cpp KatStage; the contract: include/dogeray_amd.h "known-answer
hooks"), on the generated scene of tests/shade_cases.py and n = 0, 1 and 257 items only:
  (a) n = 0 returns empty arrays of the documented shapes from every hook;
  (b) the result for 257 items is the result for the first 256 joined with the result for the last one, bit for bit -- a wrong count, offset or
      alignment in the staging shows here (every element is computed from its own inputs alone; tests/shade_checks.py holds the merged sampler,
      whose lanes share a loop, equal to the per-element reference, so it holds there too);
  (c) through ctypes with n = 1, a hook with one required pointer NULL returns DR_ERR_INVALID and leaves the caller's arrays alone; dr_kat_hit with
      visits NULL, and dr_kat_order_split with order NULL, succeed.
What the hooks compute is the parity tests' business (test_gpu_parity, test_gpu_shade, test_gpu_rays): no oracle here."""
import ctypes as C

import numpy as np
import pytest

import shade_cases as sc
import shade_checks as ck

pytestmark = pytest.mark.gpu

F, F64, I, U32, U64 = np.float32, np.float64, np.int32, np.uint32, np.uint64
N = 257
VIEW = "lens radius 0.3"
FRAME_SEED, STRIDE = 2 ** 32 + 7, 320

# what a wrapper returns: (dtype, shape) each, "n" the number of items ("4n": four per item, flat)
RETURNS = {
    "rng": ((F64, ("n",)),),
    "aabb": ((I, ("n",)), (F, ("n",))),
    "tri": ((F, ("n",)),),
    "node_planes": ((F, ("4n",)), (F, ("4n",))),
    "sphere": ((F, ("n",)),),
    "optics": ((F, ("n", 3)), (F, ("n", 3)), (F, ("n",))),
    "normal": ((F, ("n", 3)), (F, ("n", 3))),
    "hit": ((F, ("n",)), (I, ("n",)), (I, ("n",))),          # (with want_visits)
    "trace": ((F, ("n",)), (I, ("n",))),
    "sample": ((F, (2, "n", 3)), (U32, (2, "n", 2))),
    "outside": ((I, ("n",)),),
    "tex": ((U32, ("n",)),),
    "bounce": ((I, (2, "n")), (F, (2, "n", 3)), (F, (2, "n", 3)), (F, (2, "n", 3)), (U32, (2, "n", 2))),
    "miss": ((F, ("n", 3)),),
    "camera": ((F, (2, "n", 3)), (F, (2, "n", 3)), (U32, (2, "n", 2))),
    "store": ((I, ("n", 3)),),
}
# the output arrays of the C functions, in their order: (dtype, elements per item)
C_OUT = {
    "rng": ((F64, 1),), "aabb": ((I, 1), (F, 1)), "tri": ((F, 1),), "node_planes": ((F, 4), (F, 4)), "sphere": ((F, 1),), "optics": ((F, 3), (F, 3), (F, 1)),
    "normal": ((F, 3), (F, 3)), "hit": ((F, 1), (I, 1), (I, 1)), "trace": ((F, 1), (I, 1)), "sample": ((F, 3), (U32, 2), (F, 3), (U32, 2)),
    "outside": ((I, 1),), "tex": ((U32, 1),), "bounce": ((I, 2), (F, 6), (F, 6), (F, 6), (U32, 4)), "miss": ((F, 3),), "camera": ((F, 6), (F, 6), (U32, 4)),
    "store": ((I, 3),),
}
HOOKS = tuple(RETURNS)


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    return dogeray_amd


@pytest.fixture(scope="module")
def ctx(dr, tmp_path_factory):
    rts, tex = ck.files(tmp_path_factory)          # the files exist before this process touches the GPU
    scene = dr.Scene.load(rts, tex)
    scene.build_bvh()
    c = dr.Context(0).upload(scene)
    assert c.get_option("wide_depth") >= 1          # dr_kat_trace has its tree
    yield c
    c.close()


@pytest.fixture(scope="module")
def items():
    """hook -> its N input arrays, in the wrapper's order (which is the C function's)"""
    rng = np.random.default_rng(2024)
    objs = sc.scene_objects()
    rays = [sc.object_rays(ob, rng, 4) for ob in objs]
    pick = rng.permutation(4 * len(objs))[:N]
    idx = np.repeat(np.arange(len(objs), dtype=I), 4)[pick]
    o, d, t = (np.ascontiguousarray(np.concatenate([r[k] for r in rays])[pick], F) for k in range(3))
    seed, warm = sc.bounce_seeds(N)
    atten = sc.bounce_attens(N)
    v3 = lambda: rng.normal(size=(N, 3)).astype(F)
    k = np.arange(N)
    x, y, s = (a[:N].copy() for a in sc.camera_pixels(sc.camera_views()[VIEW]))
    return {
        "rng": [],
        "aabb": [v3(), v3(), v3() - F(1), v3() + F(1)],
        "tri": [v3(), v3(), v3(), v3(), v3()],
        "node_planes": [rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(U32), rng.normal(size=N).astype(F), rng.normal(size=N).astype(F)],
        "sphere": [v3(), v3(), v3(), rng.uniform(0.1, 2, N).astype(F)],
        "optics": [v3(), v3(), rng.uniform(0.5, 2, N).astype(F)],
        "normal": [idx, o, d, t],
        "hit": [o, d],
        "trace": [o, d],
        "sample": [seed, warm, np.array(sc.SAMPLER_KINDS, I)[k % 4]],
        "outside": [sc.outside_values()[(1 << 18) - 128:(1 << 18) + 129].copy()],
        "tex": [(k % len(sc.TEXTURES)).astype(I), rng.uniform(-3, 3, N).astype(F), rng.uniform(-3, 3, N).astype(F)],
        "bounce": [idx, o, d, t, atten, seed, warm],
        "miss": [v3(), atten],
        "camera": [x, y, s],
        "store": [sc.store_colours()[:N].copy()],
    }


def call(ctx, hook, arrays):
    """the wrapper on `arrays`, its result always a tuple"""
    if hook == "rng": out = ctx.kat_rng(12345, N)
    elif hook == "hit": out = ctx.kat_hit(*arrays, want_visits=True)
    elif hook == "trace": out = ctx.kat_trace(*arrays, 1)
    elif hook == "miss": out = ctx.kat_miss(*arrays, sc.TEX_ALBEDO, sc.MISS_BGINT)
    elif hook == "camera": out = ctx.kat_camera(sc.camera_views()[VIEW], sc.CAMERA_W, sc.CAMERA_H, FRAME_SEED, STRIDE, *arrays)
    elif hook == "store": out = ctx.kat_store(*arrays, 3)
    else: out = getattr(ctx, "kat_" + hook)(*arrays)
    return out if isinstance(out, tuple) else (out,)


def shape_of(shape, n):
    return tuple(n if k == "n" else 4 * n if k == "4n" else k for k in shape)


def check_shapes(hook, out, n):
    assert len(out) == len(RETURNS[hook])
    for a, (dt, shape) in zip(out, RETURNS[hook]):
        assert a.dtype == dt and a.shape == shape_of(shape, n), (hook, a.dtype, a.shape)


@pytest.mark.parametrize("hook", HOOKS)
def test_no_items_give_empty_arrays(ctx, items, hook):
    out = ctx.kat_rng(12345, 0) if hook == "rng" else call(ctx, hook, [a[:0] for a in items[hook]])
    check_shapes(hook, out if isinstance(out, tuple) else (out,), 0)


def test_tile_feedback_has_no_empty_call(dr, ctx):
    with pytest.raises(dr.DogerayError) as e:
        ctx.kat_tile_feedback(np.zeros(0, U32), 1, 1, 400, 0)
    assert e.value.code == dr.ERR_INVALID


@pytest.mark.parametrize("hook", [h for h in HOOKS if h != "rng"])
def test_257_items_are_256_and_one(ctx, items, hook):
    arrays = items[hook]
    assert all(len(a) == N for a in arrays)
    whole = call(ctx, hook, arrays)
    head, last = call(ctx, hook, [a[:N - 1] for a in arrays]), call(ctx, hook, [a[N - 1:] for a in arrays])
    check_shapes(hook, whole, N); check_shapes(hook, head, N - 1); check_shapes(hook, last, 1)
    for k, (w, h, l) in enumerate(zip(whole, head, last)):
        axis = [s in ("n", "4n") for s in RETURNS[hook][k][1]].index(True)
        joined = np.ascontiguousarray(np.concatenate([h, l], axis=axis))
        assert joined.tobytes() == np.ascontiguousarray(w).tobytes(), "%s: output %d of 257 items is not that of 256 and 1" % (hook, k)
    # and the hook did something with them: no output is all zeros
    assert all(w.any() for w in whole), hook


def test_the_trace_hooks_plain_variant_too(ctx, items):
    o, d = items["trace"]
    whole = ctx.kat_trace(o, d, 0)
    head, last = ctx.kat_trace(o[:N - 1], d[:N - 1], 0), ctx.kat_trace(o[N - 1:], d[N - 1:], 0)
    for w, h, l in zip(whole, head, last):
        assert np.concatenate([h, l]).tobytes() == w.tobytes()
    assert whole[0].tobytes() == ctx.kat_trace(o, d, 1)[0].tobytes() and (whole[0] > 0).mean() > 0.25


# ------------------------------------------------------------------ (c) null pointers, through ctypes
def c_args(hook, arrays, outs):
    """the C function's arguments after the context for one item: inputs `arrays`, outputs `outs`"""
    if hook == "rng": return [12345, 1] + outs
    if hook == "trace": return [1, 1] + arrays + outs
    if hook == "miss": return [1] + arrays + [sc.TEX_ALBEDO, float(sc.MISS_BGINT)] + outs
    if hook == "camera": return [sc.camera_views()[VIEW], sc.CAMERA_W, sc.CAMERA_H, FRAME_SEED, STRIDE, 1] + arrays + outs
    if hook == "store": return [1] + arrays + [3] + outs
    if hook == "tile_feedback": return [1, 1, 1, 400, 0] + arrays + outs
    if hook == "order_split": return [0, 1, 1] + arrays + outs      # kind 0: every output is written
    return [1] + arrays + outs


def as_c(a):
    return a.ctypes.data_as(C.c_void_p) if isinstance(a, np.ndarray) else a


@pytest.mark.parametrize("hook", HOOKS + ("tile_feedback", "order_split"))
def test_a_null_pointer_is_refused(dr, ctx, items, hook):
    f = getattr(dr.lib(), "dr_kat_" + hook)
    if hook == "tile_feedback":
        arrays, spec = [np.arange(64, dtype=U32)], ((U32, 1), (I, 1), (I, 2 * dr.MAX_REGIONS + 1))
    elif hook == "order_split":      # one tile, one region, the identity spelled out; the tile's word: the root
        arrays, spec = [np.zeros(1, I), np.array([0, 1], I), np.zeros(1, U32)], ((I, 1), (I, 2 * dr.MAX_REGIONS + 1), (I, 1), (U32, 2))
    else:
        arrays, spec = [np.ascontiguousarray(a[N - 1:]) for a in items[hook]], C_OUT[hook]
    fresh = lambda: [np.full(k, 0x5a, np.uint8).view(dt) for dt, k in ((dt, np.dtype(dt).itemsize * per) for dt, per in spec)]
    outs = fresh()
    args = c_args(hook, arrays, outs)
    assert f(ctx._h, *[as_c(a) for a in args]) == 0, dr.lib().dr_last_error()
    assert all(a.tobytes() != fresh()[k].tobytes() for k, a in enumerate(outs)), "a well-formed call writes every output"
    pointers = [k for k, a in enumerate(args) if isinstance(a, np.ndarray)]
    assert len(pointers) == len(arrays) + len(outs) + (hook == "camera")
    for k in pointers:
        outs = fresh()
        args = c_args(hook, arrays, outs)
        optional = (hook == "hit" and args[k] is outs[2]) or (hook == "order_split" and args[k] is arrays[0])
        args[k] = None
        rc = f(ctx._h, *[as_c(a) for a in args])
        if optional:
            assert rc == 0 and outs[0].tobytes() != fresh()[0].tobytes()          # visits may be NULL, and the split's order
            continue
        assert rc == dr.ERR_INVALID and dr.lib().dr_last_error() == b"null argument", (hook, k, rc)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(outs, fresh())), "a refused call leaves the caller's arrays alone"
