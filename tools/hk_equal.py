"""Two builds of tools/libhostkernel.so, entry by entry: every scene-taking entry and the accumulator stages on fixed inputs over three committed
scenes, every output buffer and return code byte for byte, one refused call per entry with its hk_last_error, and the two export lists.
    python tools/hk_equal.py OLD.so NEW.so [--time]     (from the repo root; a line per call, "equal" or "DIFFERENT"; exit status 1 on any difference)
An OLD build that still has hk_denoise_m2 / hk_reproject_m2 is matched by role: those are what hk_denoise / hk_reproject are now.
--time: Scene.render's loop instead (suzane.rts, 256 x 160, wide walk, one thread), the two builds alternating, seven runs each, counters off and on."""
import ctypes as C
import os
import subprocess
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_kernel as hk      # noqa: E402
import dogeray_amd as dr      # noqa: E402  (the scenes' own settings, by the product's reader; no GPU)

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
W, H, N = 64, 40, 512
i32, i64, u8, u32, u64, f32 = np.int32, np.int64, np.uint8, np.uint32, np.uint64, np.float32


def load(path):
    L = C.CDLL(os.path.abspath(path))
    for new, old in (("hk_denoise", "hk_denoise_m2"), ("hk_reproject", "hk_reproject_m2")):
        if hasattr(L, old):
            setattr(L, new, getattr(L, old))
    return hk.bind(L)


def z(shape, dtype=f32):
    return np.zeros(shape, dtype)


def call(L, label, name, *args, refuse=True):
    """the entry on args (arrays by address), then the same call without its first argument: (label, return code, arrays' bytes, error text) each"""
    for tag, a in (("", args), ("[null]", (None,) + args[1:]))[:2 if refuse else 1]:
        rc = getattr(L, name)(*[x.ctypes.data if isinstance(x, np.ndarray) else x for x in a])
        yield " ".join(x for x in (name, label, tag) if x), rc, [x.tobytes() for x in a if isinstance(x, np.ndarray)], L.hk_last_error() if rc < 0 else b""


def entries(L, scene):
    rng = np.random.default_rng(7)
    s = dr.Scene.load(os.path.join(GOLDEN, "scenes", scene), os.path.join(GOLDEN, "textures"))
    st, bg = dr.pack_settings13(s.settings(), 1), float(s.settings().background)
    h = L.hk_scene_load(os.fsencode(os.path.join(GOLDEN, "scenes", scene)), os.fsencode(os.path.join(GOLDEN, "textures")))
    tiles = (W // 8) * (H // 8)
    o, d = (rng.random((N, 3), f32) * 12 - 6), (rng.random((N, 3), f32) - 0.5)
    d[:6] = np.concatenate([np.eye(3), -np.eye(3)])                      # axis-parallel directions
    tmax = (rng.random(N, f32) * 30)
    tmax[::7] = 0
    seeds, skip = rng.integers(0, 2 ** 63, N).astype(u64), rng.integers(0, 9, N).astype(i32)
    view = (h, st, W, H)
    yield from call(L, "before hk_camera_entry", "hk_camera_entry_check", *view, 1, 0, 5, 3, 1, 2, z(tiles, i32), z(4, i64))
    yield "hk_has_wide / hk_wide_depth", (L.hk_has_wide(h), L.hk_wide_depth(h)), [], b""
    mu = z(3)
    yield from call(L, "", "hk_wide_mu", h, mu)
    nprims = L.hk_nearest_prims(h, *[None] * 7)
    yield from call(L, "", "hk_nearest_prims", h, z(nprims, i32), z((nprims, 3)), z((nprims, 3)), z((nprims, 3)), z(nprims, i32), z(nprims, i32), z(1))
    for tree in (1, 2, 3):
        yield from call(L, "tree %d" % tree, "hk_wide_info", h, tree, z(3, i32))
        for walk in (0, 2):
            yield from call(L, "walk %d tree %d" % (walk, tree), "hk_nearest_records", h, walk, tree)
            yield from call(L, "walk %d tree %d" % (walk, tree), "hk_nearest", h, walk, tree, N, o, tmax, z(N), z(N), z(N, i32), z(N, i32), z((N, 3)), z((N, 2)), z(N, i32), 2)
            for zm in (0, 1):
                yield from call(L, "walk %d tree %d zero_margin %d" % (walk, tree, zm), "hk_allhits", h, walk, tree, N, o, d, tmax, 4, 3, zm, z(N, i32), z((N, 4)),
                                z((N, 4), i32), z((N, 4), i32), z((N, 4)), z((N, 4, 3)), z((N, 4, 2)), z((N, 4, 3)), z(N, i32), 2)
        for trav in (0, 1, 2):
            yield from call(L, "traversal %d tree %d" % (trav, tree), "hk_hit", h, trav, tree, N, o, d, z(N), z(N, i32), z(N, i32))
            yield from call(L, "traversal %d tree %d" % (trav, tree), "hk_radiance", h, trav, tree, N, o, d, seeds, skip, 2, 5, bg, int(st[12]), 11, z((N, 3)), z(N, i32))
            t, slot = z(N), z(N, i32)
            for mode in (0, 1):
                yield from call(L, "traversal %d tree %d mode %d" % (trav, tree, mode), "hk_trace", h, trav, tree, mode, N, o, d, tmax, t, z(N, i32), z(N, i32), slot, z(N, i32))
            yield from call(L, "traversal %d tree %d" % (trav, tree), "hk_ray_surface", h, tree, N, o, d, t, slot, z(N, i32), z(N), z((N, 3)), z((N, 2)), z((N, 3)))
    yield from call(L, "", "hk_nearest_brute", h, N, o, tmax, z(N), z(N), z(N, i32), z(N, i32), z((N, 3)), z((N, 2)), 2)
    yield from call(L, "", "hk_allhits_brute", h, N, o, d, tmax, 4, 3, z(N, i32), z((N, 4)), z((N, 4), i32), 2)
    yield from call(L, "", "hk_kat_tex", h, N, z(N, i32), rng.random(N, f32), rng.random(N, f32), z(N, u32))
    yield from call(L, "", "hk_kat_bounce", h, N, rng.integers(0, nprims, N).astype(i32), o, d, tmax + 1, rng.random((N, 3), f32), seeds, skip, z((2, N), i32),
                    z((2, N, 3)), z((2, N, 3)), z((2, N, 3)), z((2, N, 2), u32))      # (both forms of the step: a leading axis of 2)
    yield from call(L, "", "hk_kat_miss", h, N, d, rng.random((N, 3), f32), int(st[12]), bg, z((N, 3)))
    n_leaves = L.hk_wide_leaves(h, None, None, None, 0, 0)
    yield from call(L, "", "hk_wide_leaves", h, z(n_leaves, u32), z((n_leaves, 6)), z((2 * n_leaves, 2), u32), n_leaves, 2 * n_leaves)
    # the 64 x 40 view of the scene's own settings
    yield from call(L, "", "hk_cert_check", *view, 40e-4, float(mu[0]) if mu[0] > 0 else 1e30, 20000, 3, z(8, i64), z((tiles + 31) // 32 + 2, u32))
    plane, codes = z(tiles, u8), z(tiles, i32)
    yield from call(L, "", "hk_cert_levels", *view, 40, 1, float(mu[0]) if mu[0] > 0 else 1e30, 20000, 3, z(24, i64), plane)
    yield from call(L, "", "hk_camera_entry", *view, 1, 0, 0, codes, z(32, i64))
    yield from call(L, "", "hk_camera_entry_check", *view, 1, 0, 5, 3, 1, 2, codes, z(4, i64))
    pix = np.arange(N, dtype=i32)
    yield from call(L, "", "hk_sky_pixel", *view, bg, 5, 3, 2, N, pix % W, pix % H, z((N, 3), i32))
    yield from call(L, "", "hk_sky_units_render", *view, bg, 5, 3, 4, 2, tiles, np.arange(tiles, dtype=i32), None, z((W, H, 3), i32), z(tiles * 64, u32))
    for trav in (0, 1, 2):
        for ctr in (z(6, u64), None):
            yield from call(L, "traversal %d counters %s" % (trav, "off" if ctr is None else "on"), "hk_render", *view, bg, 9, trav, 2, 1, 0, z((W, H, 3), i32), ctr, None, 40, 1, None)
    yield from call(L, "level plane", "hk_render", *view, bg, 9, 2, 2, 1, 0, z((W, H, 3), i32), z(6, u64), plane, 40, 1, None)
    yield from call(L, "entry plane", "hk_render", *view, bg, 9, 2, 2, 1, 0, z((W, H, 3), i32), None, None, 40, 1, codes)
    guides = {}
    for key, div, move in (("full", 1, 0.0), ("low", 2, 0.0), ("moved", 1, 0.05)):
        v = st.copy()
        v[11], v[0] = div, v[0] + move
        gh, gw = H // div // 8 * 8, W // div // 8 * 8
        g = guides[key] = hk._channels((gh, gw), hk._AOV_CHANNELS)
        for trav in (0, 1, 2):
            yield from call(L, "%s traversal %d" % (key, trav), "hk_aov", h, v, W, H, 0, 0, gw, gh, trav, 2, *[g[k] for k in hk._AOV_CHANNELS])
        g["st"] = v
    L.hk_scene_free(h)
    # the accumulator stages on a seeded accumulator with hk_aov's guides
    acc, hist, m2 = rng.integers(0, 4 * 255, (W, H, 3)).astype(i32), rng.integers(0, 8, (W, H)).astype(i32), rng.integers(0, 2 ** 40, (W, H)).astype(u64)
    F, Lo, M = guides["full"], guides["low"], guides["moved"]
    four = lambda g: [g[k] for k in ("normal", "albedo", "depth", "material")]
    yield from call(L, "", "hk_denoise", acc, W, H, 4, st, *four(F), None, z((H, W, 3)), z((H, W, 3), u8), 2, hist, m2)
    yield from call(L, "", "hk_upscale", acc, W, H, 4, Lo["st"], *four(Lo), *four(F), None, hk._denoise_raw(hk.DENOISE_DEFAULTS), z((H, W, 3)), z((H, W, 3), u8), z((H, W), u8), 2, hist, m2)
    yield from call(L, "", "hk_reproject", acc, hist, W, H, 4, st, M["st"], F["t"], F["normal"], F["material"], M["t"], M["normal"], M["material"], None,
                    z((W, H, 3), i32), z((W, H), i32), z(5, i64), 2, m2, z((W, H), u64))
    yield from call(L, "", "hk_error", acc, hist, m2, W, H, 4, 0.05, st, z((H, W)), z(19, u64), z(2, i32), 2)
    yield from call(L, "", "hk_moments_add", acc.copy(), rng.integers(0, 255, (W, H, 3)).astype(i32), m2.copy(), W * H)


def exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " hk_" in line}


def render_times(libs):
    s = dr.Scene.load(os.path.join(GOLDEN, "scenes", "suzane.rts"), "")
    st, out = dr.pack_settings13(s.settings(), 1), z((256, 160, 3), i32)
    hs = [L.hk_scene_load(os.fsencode(os.path.join(GOLDEN, "scenes", "suzane.rts")), b"") for L in libs]
    for ctr in (None, z(6, u64)):
        t = [[], []]
        for k in range(16):                                                  # (the first pair warms up)
            t0 = time.perf_counter()
            libs[k % 2].hk_render(hs[k % 2], st.ctypes.data, 256, 160, 1.0, 9, 2, 1, 1, 0, out.ctypes.data, None if ctr is None else ctr.ctypes.data, None, 40, 1, None)
            if k >= 2:
                t[k % 2].append(time.perf_counter() - t0)
        med, spread = [sorted(x)[3] for x in t], max(t[0]) - min(t[0])
        print("render count=%s: old %s | new %s | medians %.4f %.4f s, old spread %.4f s: %s" % (ctr is not None, " ".join("%.4f" % x for x in t[0]),
              " ".join("%.4f" % x for x in t[1]), med[0], med[1], spread, "within" if med[1] <= med[0] + spread else "SLOWER"))


if __name__ == "__main__":
    old, new = sys.argv[1], sys.argv[2]
    libs = [load(old), load(new)]
    if "--time" in sys.argv:
        sys.exit(render_times(libs))
    bad = 0
    for scene in ("cube.rts", "glass.rts", "suzane.rts"):
        for a, b in zip(entries(libs[0], scene), entries(libs[1], scene)):
            bad += a != b
            print("%s %s: %s (return %r / %r, %d bytes, crc %08x, %r / %r)" % (scene, a[0], "equal" if a == b else "DIFFERENT", a[1], b[1], sum(map(len, b[2])),
                                                                              zlib.crc32(b"".join(b[2])), a[3].decode(), b[3].decode()))
    gone, came = sorted(exports(old) - exports(new)), sorted(exports(new) - exports(old))
    print("exports only in old: %s; only in new: %s" % (" ".join(gone) or "none", " ".join(came) or "none"))
    sys.exit(1 if bad or came or set(gone) - {"hk_denoise_m2", "hk_reproject_m2"} else 0)
