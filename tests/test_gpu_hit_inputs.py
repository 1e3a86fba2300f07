"""What the lean persistent build hands its shade phase about a hit (device_prims.hpp HIT_UV_CARRIED, HIT_FETCH_LAZY: the barycentrics carried from
the leaf step in two stash words, the primitive record and the texture coordinates fetched only where read), on the GPU.  Every render runs the lean
build (coop_tiles_per_wave = 0) with two frames per launch, as tests/test_gpu_camera_cert.py forces it, and is compared pixel for pixel with the
oracle and with the same library's counting build, which keeps the plain shade path: the same frames through the old code.  Before a scene is rendered
its records are checked, from the file alone, to hold the classes the test names."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import with_settings

pytestmark = pytest.mark.gpu

SCENES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes")
SEED, STRIDE, FRAMES = 7, 1000003, 2


@pytest.fixture(scope="module")
def dr():
    import dogeray_amd
    assert dogeray_amd.device_count() >= 1
    return dogeray_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


@pytest.fixture(scope="module")
def ctx(dr, synth):          # synth first: the generated scenes exist before this process touches the GPU
    c = dr.Context(0)
    c.set_option("coop_tiles_per_wave", 0)      # every launch runs the lean build
    yield c
    c.close()


def classes_of(path):
    """The classes of record in a .rts file, from its text alone (columns as csrc/rts_reader.cpp reads them)"""
    found = set()
    for line in open(path).read().split("\n"):
        c = line.strip().split(",")
        if len(c) < 13 or c[0].startswith("*"):
            continue
        kind = int(float(c[3]))
        if kind == 0:
            found.add("sphere")
        if kind != 2:
            continue
        found.add("triangle")
        found.add("sentinel" if len(c) < 19 or float(c[18]) == -20 else "file normal")
        smooth = len(c) > 34 and int(float(c[34])) == 1
        found.add("smooth on" if smooth else "smooth off")
        if len(c) > 35 and int(float(c[35])) == 1: found.add("checker")
        if len(c) > 36 and c[36].strip() != "no": found.add("textured")
        if len(c) > 37 and c[37].strip() != "no": found.add("roughness texture")
    return found


def check_scene(dr, orc, ctx, path, texdir, W, H, needs, seed=SEED):
    have = classes_of(path)
    assert set(needs) <= have, "%s holds %s, the test names %s" % (os.path.basename(path), sorted(have), sorted(needs))
    sc = dr.Scene.load(path, texdir); sc.build_bvh()
    ctx.upload(sc)
    s = sc.settings()
    st = dr.pack_settings13(s, 1)
    os_ = orc.Scene(path, texdir or None); os_.build_bvh()
    ref = sum(os_.render(st, W, H, s.background, seed + STRIDE * k, nthreads=8)[0].astype(np.int64) for k in range(FRAMES))
    out = []
    for counting in (False, True):
        ctx.enable_counters(counting)
        ctx.accum_reset(W, H)
        ctx.render_accumulate(st, W, H, s.background, seed, STRIDE, FRAMES)
        out.append(ctx.accum_read().astype(np.int64))
    ctx.enable_counters(False)
    lean, counting = out
    assert ref.any()
    bad = np.argwhere(np.any(lean != counting, axis=2))
    assert len(bad) == 0, "%s: lean and counting builds differ at %d pixels, first %r" % (os.path.basename(path), len(bad), bad[:4].tolist())
    bad = np.argwhere(np.any(lean != ref, axis=2))
    assert len(bad) == 0, "%s: lean build and oracle differ at %d pixels, first %r" % (os.path.basename(path), len(bad), bad[:4].tolist())


def test_heightfield_with_smooth_normals(dr, orc, ctx, synth, tmp_path):
    src = os.path.join(synth["dir"], "hf_small.rts")
    path = with_settings(src, str(tmp_path / "hf64.rts"), [l for l in open(src).read().split("\n") if l.startswith("*")][0])
    check_scene(dr, orc, ctx, path, "", 64, 48, ("triangle", "file normal", "smooth on"))


def test_spheres_and_triangles_mixed(dr, orc, ctx, synth):
    check_scene(dr, orc, ctx, os.path.join(synth["dir"], "matball.rts"), synth["tex"], 64, 48, ("sphere", "triangle"))
    check_scene(dr, orc, ctx, os.path.join(SCENES, "scene.rts"), "", 64, 48, ("sphere",))


def test_bolter_with_its_two_textures(dr, orc, ctx, tmp_path):
    import reference_image as ri
    path, texdir = ri.bolter_scene(tmp_path)
    check_scene(dr, orc, ctx, path, texdir, 64, 48, ("triangle", "textured", "smooth on"))


def test_checker_and_roughness_texture(dr, orc, ctx, synth):
    check_scene(dr, orc, ctx, os.path.join(SCENES, "textest.rts"), synth["tex"], 64, 48, ("triangle",))
    check_scene(dr, orc, ctx, os.path.join(SCENES, "rough.blend.rts"), synth["tex"], 64, 48, ("triangle", "roughness texture"))


def test_sentinel_face_normals(dr, orc, ctx, tmp_path):
    """Triangles without a face normal in the file (16 columns: the -20 sentinel, the cross product is used) beside triangles with one, and the
    sentinel written out with vertex normals and the smooth flag behind it (never followed: K:748)."""
    rng = np.random.default_rng(3)
    lines = ["*,0.0,-1.0,6.0,0.01,0,0,0,5,50,5,1,1,no,64,48"]
    for k in range(120):
        v0 = rng.uniform(-2.5, 2.5, 3); v1 = v0 + rng.uniform(-1.2, 1.2, 3); v2 = v0 + rng.uniform(-1.2, 1.2, 3)
        cols = ["%f" % v for v in v0] + ["2"] + ["%f" % v for v in rng.uniform(0.2, 1, 3)] + ["0.3", "0"] + ["%f" % v for v in v1] + [str((0, 2, 3, 5)[k % 4])] + ["%f" % v for v in v2]
        if k % 3 == 1:
            cols += ["0.0", "0.0", "-20.0"] + ["%f" % v for v in rng.normal(size=9)] + ["0", "0", "1", "0", "0", "1"] + ["1", "0"]
        elif k % 3 == 2:
            n = np.cross(v1 - v0, v2 - v0); n /= np.linalg.norm(n)
            cols += ["%f" % v for v in n]
        lines.append(",".join(cols))
    path = tmp_path / "sentinel.rts"
    path.write_text("\n".join(lines) + "\n")
    check_scene(dr, orc, ctx, str(path), "", 64, 48, ("triangle", "sentinel", "file normal", "smooth on", "smooth off"))


def test_fuzz_slice(dr, orc, ctx, synth, tmp_path):
    """Three dozen of the suite's small random scenes (scene_fuzz.random_scene: spheres, every material, textures, checker flags, coincident
    triangles -- a walk improves its best hit more than once and meets ties on t --, zero-area triangles, four scales)."""
    from scene_fuzz import random_scene
    rng = np.random.default_rng(4242)
    names = ["synth_albedo.ppm", "synth_rough.ppm", "synth_env.ppm", "a.ppm"]
    seen = set()
    for k in range(36):
        n = int(rng.integers(2, 400))
        path = random_scene(rng, n, str(tmp_path / ("fuzz%d.rts" % k)), W=64, H=48, textures=names, scale=(1.0, 0.05, 1.0, 0.02)[k % 4])
        body = [l for l in open(path).read().split("\n") if l and not l.startswith("*")]
        if len({l.split(",", 7)[0:3].__repr__() + l.split(",")[9] for l in body}) < len(body): seen.add("coincident")
        seen |= classes_of(path)
        check_scene(dr, orc, ctx, path, synth["tex"], 64, 48, (), seed=100 + k)
    assert {"coincident", "sphere", "sentinel", "file normal", "textured", "roughness texture", "checker", "smooth on", "smooth off"} <= seen, sorted(seen)
