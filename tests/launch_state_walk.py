"""One scripted walk through the transitions of what a render launch caches per view (dogeray_amd/csrc/launch_state.hpp: the tile order, the camera
rays' tile words, the sky split), for tests/test_gpu_launch_state.py.  prepare() makes the scenes, the oracle's frames and the host build's entry tables
-- before the process touches the GPU --; steps() walks one context and yields after every step what the context answers and what the step implies.

The walk (frames of 64 x 64 unless said, every step on a fresh accumulator, seeds SEED + k STRIDE):
   1  view A, 8 frames in one launch                 the table and the split are computed, the order is made
   2  A again                                        ... and reused
   3  view B, one frame                              first sight of a single-frame view: no table is computed -- the launch reads none (no split)
                                                     and dr_stats_camera_entry still answers the last computed one, A's -- and the order follows the camera
   4  B, one frame again                             B's table
   5  camera_entry 0, then 1                         no table, then A's again
   6  cert_levels 0, then 1                          the words are recomputed (neither scene has triangles with own bounds: no certificate either way)
   7  sky_tiles 0, 1, 2                              no split, the kernel in front, the retiring waves
   8  feedback 0, then 1                             no order, then a new one
   9  stripe (2, 1) and back                         another tile grid: 32 tiles
  10  128 x 64                                       128 tiles
  11  the second scene, view A's settings unchanged  the order survives the upload, the table does not
  12  24 frames through the pipeline (groups of 8)   two launches that refresh the order and one that holds it; per-frame stores are not split
  13  an ordinary launch                             reuses the pipeline's table, and splits
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

SEED, STRIDE = 41, 1000003
NUM_CUS = 256          # of an MI355X (the feedback's split limit is made from it)


def _tiles(W, H, mod=1, rem=0):
    gx, gy = W // 8, H // 8
    return ((gx - rem + mod - 1) // mod if gx > rem else 0) * gy


def prepare(dr, synth):
    """{scene name: {"scene", "bg", "A", "B", ("oracle", view, W, H, mod, rem): [frames], ("entry", view, W, H, mod, rem): codes, "certificate": bool}}"""
    import host_kernel
    from oracle import orc
    need = {"hf_small": (("A", 64, 64, 1, 0, 8), ("B", 64, 64, 1, 0, 1), ("A", 64, 64, 2, 1, 2), ("A", 128, 64, 1, 0, 2)),
            "city_small": (("A", 128, 64, 1, 0, 2), ("A", 64, 64, 1, 0, 24))}
    world = {}
    for name, configs in need.items():
        path = os.path.join(synth["dir"], name + ".rts")
        sc = dr.Scene.load(path, ""); sc.build_bvh()
        s = sc.settings()
        a = world["hf_small"]["A"] if world else dr.pack_settings13(s, 1, spp=1)      # one view A for both scenes: step 11 changes the scene alone
        b = a.copy(); b[0] += np.float32(3.0)          # the eye moves sideways
        hs = host_kernel.Scene(path, "")
        own, mu = hs.wide_mu()
        o = orc.Scene(path, None); o.build_bvh()
        e = {"scene": sc, "bg": s.background, "A": a, "B": b, "certificate": own > 0 and float(mu[0]) > 0.0}
        for view, W, H, mod, rem, frames in configs:
            st = e[view]
            fr = [o.render(st, W, H, s.background, SEED + STRIDE * k, nthreads=8, col_mod=mod, col_rem=rem)[0].astype(np.int64) for k in range(frames)]
            for f in fr: f.flags.writeable = False
            e["oracle", view, W, H, mod, rem] = fr
            table = hs.camera_entry(st, W, H, mod, rem)
            assert table is not None and len(table[0]) == _tiles(W, H, mod, rem), "the walk's views have entry tables"
            e["entry", view, W, H, mod, rem] = table[0]
        o.close()
        world[name] = e
    hf = world["hf_small"]
    assert 0 < int((hf["entry", "A", 64, 64, 1, 0] == -1).sum()) < 64, "view A has sky tiles and others"
    assert not np.array_equal(hf["entry", "A", 64, 64, 1, 0], hf["entry", "B", 64, 64, 1, 0]), "the views' tables differ"
    assert np.array_equal(world["city_small"]["A"], hf["A"]) and not np.array_equal(world["city_small"]["entry", "A", 128, 64, 1, 0], hf["entry", "A", 128, 64, 1, 0])
    return world


def steps(ctx, world):
    """walks `ctx` (a fresh context); yields per step a dict: label, acc / want_acc, entry / want_entry (None: no table), levels (the read-back's
    length) / want_levels, sky / want_sky, order (tile_order()'s ntiles, regions, heavy_factor, split_steps, split_limit and the order's length, or
    None) / want_order"""
    import host_kernel
    ctx.set_option("coop_tiles_per_wave", 0)      # every launch runs the lean build: the one that reads the tiles' words and is split
    ctx.set_option("pipe_group", 8)
    limit = host_kernel.plan_split_limit(NUM_CUS, ctx.get_option("occupancy"), ctx.get_option("split_parts"), ctx.get_option("split_waves"))
    heavy, split_steps = ctx.get_option("heavy_factor"), ctx.get_option("split_steps")
    state = {"scene": "hf_small", "stripe": (1, 0)}
    ctx.upload(world["hf_small"]["scene"])

    def launch(label, view, W, H, frames, table, split, order=True, pipelined=False):
        """table: the view whose table the context answers afterwards (None: none); split: the view whose table the launch was split by (None: not split)"""
        e = world[state["scene"]]
        mod, rem = state["stripe"]
        ctx.accum_reset(W, H)
        (ctx.render_accumulate_pipelined if pipelined else ctx.render_accumulate)(e[view], W, H, e["bg"], SEED, STRIDE, frames)
        acc = ctx.accum_read().astype(np.int64)
        tiles = _tiles(W, H, mod, rem)
        live = ctx.tile_order()
        want_sky = (0, 0)
        if split is not None:
            n_none = int((e["entry", split, W, H, mod, rem] == -1).sum())
            want_sky = (n_none, tiles - n_none)
        entry = ctx.camera_entry()
        return {"label": label, "acc": acc, "want_acc": sum(e["oracle", view, W, H, mod, rem][:frames]),
                "entry": entry if len(entry) else None, "want_entry": None if table is None else e["entry", table, W, H, mod, rem],
                "levels": len(ctx.cert_levels()), "want_levels": tiles if e["certificate"] and table is not None and ctx.get_option("camera_cert") else 0,
                "sky": ctx.sky_tiles(), "want_sky": want_sky,
                "order": None if live is None else (live["ntiles"], live["regions"], live["heavy_factor"], live["split_steps"], live["split_limit"], len(live["order"])),
                "want_order": (tiles, 1, heavy, split_steps, limit, tiles) if order else None}

    yield launch("1 view A, 8 frames", "A", 64, 64, 8, "A", "A")
    yield launch("2 A again", "A", 64, 64, 8, "A", "A")
    yield launch("3 view B, one frame: first sight", "B", 64, 64, 1, "A", None)
    yield launch("4 B again", "B", 64, 64, 1, "B", "B")
    ctx.set_option("camera_entry", 0)
    yield launch("5 camera_entry 0", "A", 64, 64, 2, None, None)
    ctx.set_option("camera_entry", 1)
    yield launch("5 camera_entry 1", "A", 64, 64, 2, "A", "A")
    for v in (0, 1):
        ctx.set_option("cert_levels", v)
        yield launch("6 cert_levels %d" % v, "A", 64, 64, 2, "A", "A")
    for v in (0, 1, 2):
        ctx.set_option("sky_tiles", v)
        yield launch("7 sky_tiles %d" % v, "A", 64, 64, 2, "A", "A" if v else None)
    ctx.set_option("feedback", 0)
    yield launch("8 feedback 0", "A", 64, 64, 2, "A", "A", order=False)
    ctx.set_option("feedback", 1)
    yield launch("8 feedback 1", "A", 64, 64, 2, "A", "A")
    ctx.set_stripe(2, 1); state["stripe"] = (2, 1)
    yield launch("9 stripe (2, 1)", "A", 64, 64, 2, "A", "A")
    ctx.set_stripe(1, 0); state["stripe"] = (1, 0)
    yield launch("9 stripe (1, 0)", "A", 64, 64, 2, "A", "A")
    yield launch("10 128 x 64", "A", 128, 64, 2, "A", "A")
    ctx.upload(world["city_small"]["scene"]); state["scene"] = "city_small"
    yield launch("11 the second scene", "A", 128, 64, 2, "A", "A")
    yield launch("12 three pipelined groups", "A", 64, 64, 24, "A", None, pipelined=True)
    yield launch("13 an ordinary launch", "A", 64, 64, 2, "A", "A")
