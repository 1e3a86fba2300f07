"""The camera rays' entry table (option camera_entry) on the host build of the kernel's own code (tools/host_kernel.cpp: the same
entry_leaf / entry_tile / cert_box_rect the device runs):
 * soundness by brute force -- the kernel's real camera rays (camera_ray, the frames' seeds) against EVERY leaf of the tree: a leaf whose padded box a
   ray enters (slab(), the reference's test; on a sample of pairs it is held against the oracle's own aabb) lies under the entry of the ray's tile;
 * frames rendered from the entries equal the frames rendered from the root and the oracle's, the rays are the same and the records fewer;
 * the corners (camera inside the scene, a tile without geometry, a tile with one leaf, stripes, a NaN vertex) and four wrong rules, each caught.
No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tools"))
import camera_entry_cases as cases
import ray_cases
from camera_entry_cases import FRAMES, SEED, SIZES, STRIDE


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    return dogeray_amd


@pytest.fixture(scope="module")
def paths(synth, tmp_path_factory):
    return cases.paths(synth, tmp_path_factory.mktemp("entry"))


_loaded = {}


def _scene(dr, paths, name):
    """(host build's scene, settings, settings13 at one sample per pixel), loaded once; None when the scene has no wide tree"""
    import host_kernel
    if name not in _loaded:
        path, tex = paths[name]
        hs = host_kernel.Scene(path, tex)
        s = dr.Scene.load(path, tex).settings()
        _loaded[name] = (hs, s, dr.pack_settings13(s, 1, spp=1)) if hs.wide_info(2)["wide_depth"] > 0 else None
    return _loaded[name]


def test_every_entered_leaf_lies_under_its_tiles_entry(dr, paths):
    from oracle import orc
    import host_kernel
    checked = 0
    shares = {}
    rng = np.random.default_rng(3)
    both = False
    for name in sorted(paths):
        e = _scene(dr, paths, name)
        if e is None:
            continue                                   # (far_refused: no wide tree, nothing to enter)
        hs, s, st0 = e
        for st1 in cases.views(name, st0):
            for k in range(3):
                st = cases.lens(st1, k)
                for W, H in SIZES:
                    table = hs.camera_entry(st, W, H)
                    if table is None:
                        continue                       # (a lens too wide for its focus plane: the view gives no table, every ray starts at the root)
                    codes, c = table
                    got = hs.camera_entry_check(st, W, H, codes, SEED, STRIDE, FRAMES)
                    assert got["rays"] == (W // 8) * (H // 8) * 64 * FRAMES
                    assert got["outside"] == 0, (name, k, W, H, got, c)
                    geo = c["tiles"] - c["none"]
                    shares.setdefault(name, []).append((c["root"], geo, c["none"], got["entered_below_root"]))
                    checked += 1
        # the listing itself, on a sample: slab() against the oracle's aabb for this scene's rays and leaf boxes
        rec, boxes, _ = hs.wide_leaves()
        n = 2000
        o = np.tile(np.array(st0[0:3], np.float32), (n, 1))
        pick = rng.integers(0, len(boxes), n)
        target = boxes[pick, 0:3] + (boxes[pick, 3:6] - boxes[pick, 0:3]) * rng.uniform(-0.3, 1.3, (n, 3)).astype(np.float32)
        d = (target - o).astype(np.float32)
        hit, _ = orc.kat_aabb(o, d, boxes[pick, 0:3], boxes[pick, 3:6])
        assert np.array_equal(hit != 0, host_kernel.slab(o, d, boxes[pick, 0:3], boxes[pick, 3:6]) != 0), name
        both = both or 0.05 < (hit != 0).mean() < 0.95   # aimed at the boxes and around them: both outcomes
    assert both
    for name, rows in sorted(shares.items()):
        root, geo = sum(r[0] for r in rows), sum(r[1] for r in rows)
        print("%-14s tiles that see geometry %5d, of them at the root %5d (%.0f %%), tiles without geometry %5d, leaves entered below the root %d" %
              (name, geo, root, 100.0 * root / max(1, geo), sum(r[2] for r in rows), sum(r[3] for r in rows)))
    assert checked >= 100
    # a scene proves something only where tiles leave the root: looking down on hf_small at least half of the geometry tiles must
    for name in ("hf_1", "hf_0.1"):
        hs, s, st0 = _scene(dr, paths, name)
        for W, H in SIZES:
            codes, c = hs.camera_entry(cases.top(name, st0), W, H)
            geo = c["tiles"] - c["none"]
            assert geo > 0 and 2 * (geo - c["root"]) >= geo, (name, W, H, c)
            assert hs.camera_entry_check(cases.top(name, st0), W, H, codes, SEED, STRIDE, FRAMES)["entered_below_root"] > 0


_oracle = {}


def _reference(paths, name, st, W, H, bg):
    key = (name, st.tobytes(), W, H)
    if key not in _oracle:
        from oracle import orc
        o = orc.Scene(paths[name][0], paths[name][1] or None)
        o.build_bvh()
        _oracle[key] = o.render(st, W, H, bg, SEED, nthreads=8)
        _oracle[key][0].setflags(write=False)
    return _oracle[key]


@pytest.mark.parametrize("name", cases.NAMED)
def test_frames_from_the_entries_are_the_frames_from_the_root(dr, paths, name):
    hs, s, st0 = _scene(dr, paths, name)
    for st in cases.views(name, st0):
        for W, H in SIZES:
            codes, c = hs.camera_entry(st, W, H)
            root, cr = hs.render(st, W, H, s.background, SEED, nthreads=8, entry_plane=np.zeros_like(codes))
            entry, ce = hs.render(st, W, H, s.background, SEED, nthreads=8, entry_plane=codes)
            want, co = _reference(paths, name, st, W, H, s.background)
            assert np.array_equal(entry, root) and np.array_equal(entry, want), (name, W, H)
            assert ce["rays"] == cr["rays"] == co["rays"]
            assert ce["V"] <= cr["V"]
            if name.startswith("hf_"):
                print("%s %dx%d: records per ray %.3f from the root, %.3f from the entries" % (name, W, H, cr["V"] / cr["rays"], ce["V"] / ce["rays"]))
                assert ce["V"] < cr["V"], (name, W, H, c)


def test_every_scene_renders_the_same_from_its_entries(dr, paths):
    """the adversarial scenes of tests/ray_cases.py: the frame from the entries is the frame from the root"""
    n = 0
    for name in sorted(paths):
        e = _scene(dr, paths, name)
        if e is None:
            continue
        hs, s, st = e
        W, H = SIZES[1]
        table = hs.camera_entry(st, W, H)
        assert table is not None, name
        root, cr = hs.render(st, W, H, s.background, SEED, nthreads=8, entry_plane=np.zeros_like(table[0]))
        entry, ce = hs.render(st, W, H, s.background, SEED, nthreads=8, entry_plane=table[0])
        assert np.array_equal(entry, root) and ce["rays"] == cr["rays"] and ce["V"] <= cr["V"], name
        n += 1
    assert n >= 15


def test_camera_inside_the_scene_keeps_every_tile_at_the_root(dr, paths):
    hs, s, st0 = _scene(dr, paths, "hf_1")
    st = st0.copy()
    st[0:3] = st[3:6]; st[0] += np.float32(0.05)            # the eye at the look-at point, in the middle of the field: leaves on every side of the lens
    codes, c = hs.camera_entry(st, 64, 40)
    assert c["every"] == 1 and c["root"] == c["tiles"] and not codes.any()
    assert hs.camera_entry_check(st, 64, 40, codes, SEED, STRIDE, 2)["outside"] == 0


def test_tiles_without_geometry_and_with_one_leaf(dr, tmp_path):
    import host_kernel
    from oracle import orc
    path = cases.one_triangle_scene(tmp_path)
    hs = host_kernel.Scene(path, "")
    s = dr.Scene.load(path, "").settings()
    st = dr.pack_settings13(s, 1, spp=1)
    W, H = 64, 40
    codes, c = hs.camera_entry(st, W, H)
    rec, boxes, rng = hs.wide_leaves()
    assert c["none"] >= c["tiles"] - 6 and c["none"] < c["tiles"]            # the triangle's box reaches a few tiles around the centre, no other does
    seen = codes[codes != -1]
    assert len(seen) and (seen & 1).all() and len(set(seen.tolist())) == 1   # one leaf: the entry is that leaf's record
    assert (seen[0] >> 1) in rec.tolist()
    got = hs.camera_entry_check(st, W, H, codes, SEED, STRIDE, FRAMES)
    assert got["outside"] == 0 and got["entered_below_root"] > 0
    root, cr = hs.render(st, W, H, s.background, SEED, entry_plane=np.zeros_like(codes))
    entry, ce = hs.render(st, W, H, s.background, SEED, entry_plane=codes)
    o = orc.Scene(path, None); o.build_bvh()
    want, co = o.render(st, W, H, s.background, SEED)
    assert np.array_equal(entry, root) and np.array_equal(entry, want)
    assert ce["rays"] == cr["rays"] == co["rays"]                            # a ray of a tile without geometry is still a ray
    assert ce["V"] < cr["V"]


@pytest.mark.parametrize("mod", [2, 3])
def test_stripes_index_the_table_by_local_columns(dr, paths, mod):
    hs, s, st0 = _scene(dr, paths, "hf_0.1")
    st = cases.top("hf_0.1", st0)
    W, H = 72, 44
    whole, _ = hs.camera_entry(st, W, H)
    gy = H // 8
    saved = 0
    for rem in range(mod):
        codes, c = hs.camera_entry(st, W, H, mod, rem)
        cols = list(range(rem, W // 8, mod))
        assert c["tiles"] == len(cols) * gy
        got = hs.camera_entry_check(st, W, H, codes, SEED, STRIDE, FRAMES, mod, rem)
        assert got["outside"] == 0 and got["rays"] == len(cols) * gy * 64 * FRAMES
        # a stripe's tile sees what the whole frame's tile sees
        for k, col in enumerate(cols):
            assert np.array_equal(codes[k * gy:(k + 1) * gy], whole[col * gy:(col + 1) * gy]), (mod, rem, col)
        a, ca = hs.render(st, W, H, s.background, SEED, col_mod=mod, col_rem=rem, entry_plane=np.zeros_like(codes))
        b, cb = hs.render(st, W, H, s.background, SEED, col_mod=mod, col_rem=rem, entry_plane=codes)
        assert np.array_equal(a, b) and ca["rays"] == cb["rays"] and cb["V"] <= ca["V"]
        saved += ca["V"] - cb["V"]
    assert saved > 0                                        # (a stripe of three columns over the middle of the field may keep all its tiles at the root)


def test_a_nan_vertex_gives_no_table_or_a_sound_one(dr, tmp_path):
    import host_kernel
    path = cases.one_triangle_scene(tmp_path)
    with open(path, "a") as f:
        f.write(ray_cases.tri_line((float("nan"), 0.0, 0.0), (0.1, 0.0, 0.0), (0.0, 0.0, 0.1)) + "\n")
    try:
        hs = host_kernel.Scene(path, "")
    except RuntimeError:
        return                                                               # the reader refuses it: nothing to walk
    st = dr.pack_settings13(dr.Scene.load(path, "").settings(), 1, spp=1)
    if hs.wide_info(2)["wide_depth"] == 0:
        return                                                               # no wide tree (the builder refuses a box that is not finite): no table
    table = hs.camera_entry(st, 64, 40)
    if table is not None:
        assert hs.camera_entry_check(st, 64, 40, table[0], SEED, STRIDE, FRAMES)["outside"] == 0


# the wrong rules (device_cert.hpp ENTRY_MUTANT) and the case that catches each
def _caught(hs, st, W, H, mutant, frames=FRAMES):
    table = hs.camera_entry(st, W, H, mutant=mutant)
    assert table is not None
    return hs.camera_entry_check(st, W, H, table[0], SEED, STRIDE, frames)["outside"]


def test_mutant_rect_narrowed_by_one_tile_is_caught(dr, paths):
    hs, s, st0 = _scene(dr, paths, "hf_0.1")
    assert _caught(hs, cases.top("hf_0.1", st0), 64, 40, 0) == 0 and _caught(hs, cases.top("hf_0.1", st0), 64, 40, 1) > 0


def test_mutant_lens_term_dropped_is_caught(dr, tmp_path):
    """one small triangle 3.6 away, the lens as wide as a view allows (a tenth of the focus distance) and focused at 1: its image is spread over a
    quarter of the focus plane's width in all -- tiles away from its pinhole image at 320 x 192"""
    import host_kernel
    path = cases.one_triangle_scene(tmp_path)
    hs = host_kernel.Scene(path, "")
    st = dr.pack_settings13(dr.Scene.load(path, "").settings(), 1, spp=1)
    st[7] = np.float32(1.0); st[6] = np.float32(0.1)
    assert _caught(hs, st, 320, 192, 0, frames=4) == 0 and _caught(hs, st, 320, 192, 2, frames=4) > 0


def test_mutant_highest_rank_off_by_one_is_caught(dr, tmp_path):
    """two leaves of consecutive ranks in one tile: with the highest rank one too low the tile's entry is the first leaf alone"""
    import host_kernel
    path = cases.pair_scene(tmp_path)
    hs = host_kernel.Scene(path, "")
    st = dr.pack_settings13(dr.Scene.load(path, "").settings(), 1, spp=1)
    assert _caught(hs, st, 64, 40, 0) == 0 and _caught(hs, st, 64, 40, 3) > 0


def test_mutant_none_where_a_leaf_exists_is_caught(dr, tmp_path):
    import host_kernel
    path = cases.one_triangle_scene(tmp_path)
    hs = host_kernel.Scene(path, "")
    st = dr.pack_settings13(dr.Scene.load(path, "").settings(), 1, spp=1)
    assert _caught(hs, st, 64, 40, 0) == 0 and _caught(hs, st, 64, 40, 4) > 0


def test_the_option_and_the_call_are_in_the_header_and_the_binding(dr):
    root = os.path.join(HERE, "..")
    hdr = open(os.path.join(root, "include", "dogeray_amd.h")).read()
    src = open(os.path.join(root, "dogeray_amd", "csrc", "context.cpp")).read()
    assert '"camera_entry"' in hdr and '"camera_entry"' in src
    assert "int dr_stats_camera_entry(dr_context* c, int32_t* out, int max, int* n_tiles);" in hdr
    assert "dr_stats_camera_entry" in dr.API_SYMBOLS and hasattr(dr.Context, "camera_entry")
