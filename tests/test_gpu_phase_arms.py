"""Every arm of the shade / refill phase in the same waves (dogeray_amd/csrc/device_shade.hpp shade_material, shade_scatter, shade_miss; the phase of
kernels_render.hip), through the lean six-wave build, byte for byte against the oracle.  One 64 x 64 scene written here: spheres and triangles side by
side, a few pixels each, of every material -- diffuse with and without add_x, emissive, mirror, metal, glass (a sphere, and triangles seen from both
sides for the ray that cannot refract), glossy, an unknown material -- and triangles with an albedo texture, a roughness texture and the checker flag;
rendered with the background texture off and on, 8 frames per launch, depth 10.

That each arm really is taken is shown on the oracle's side alone, before any GPU work: the camera rays of the launch's first frame (orc.kat_camera)
are followed through raycolor's loop composed from the oracle's functions (tests/radiance_cases.py oracle_radiance), which counts the bounces per
branch (orc.BRANCHES), the rays that miss and the paths that end at the depth limit; the object index of every hit on the way (kat_hit's) says which
objects the paths reach: every object of the scene is hit by a camera ray and by a scattered ray, and so is each arm that is a property of the object
-- emissive and the unknown material apart, a texture, a roughness texture, both, the checker flag, a sphere, a triangle (ARMS)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import radiance_cases
import shade_cases

pytestmark = pytest.mark.gpu

W, H = 64, 64
SEED, STRIDE = 31, 1000003
FRAMES = 8
BACKGROUNDS = ("no", "synth_env")


def _objects():
    def sphere(x, y, mat, add_x=0, extra=0.3, col=(0.8, 0.5, 0.3)):
        return {"type": 0, "pos": [x, y, 0.0], "radius": 0.2, "col": list(col), "extra": extra, "add_x": add_x, "mat": mat}

    def tri(x, y, mat, add_x=0, extra=0.3, flip=False, **kw):
        v0, v1, v2 = [x - 0.2, y, -0.2], [x + 0.2, y, -0.2], [x, y + 0.05, 0.25]
        if flip:
            v1, v2 = v2, v1
        o = {"type": 2, "v0": v0, "v1": v1, "v2": v2, "col": [0.6, 0.8, 0.4], "extra": extra, "add_x": add_x, "mat": mat, "norm": None, "vn": None,
             "smooth": 0, "checker": 0, "tex": "no", "rtex": "no", "tc": None}
        o.update(kw)
        return o
    xs = (-1.0, -0.5, 0.0, 0.5, 1.0)
    return [sphere(xs[0], 0.6, 0), sphere(xs[1], 0.6, 0, add_x=1), sphere(xs[2], 0.6, 1, col=(0.9, 0.9, 0.7)), sphere(xs[3], 0.6, 2), sphere(xs[4], 0.6, 3),
            sphere(xs[0], 0.0, 4, add_x=1, extra=1.5), sphere(xs[1], 0.0, 5), sphere(xs[2], 0.0, 7), tri(xs[3], 0.0, 4, add_x=1, extra=1.5),
            tri(xs[4], 0.0, 4, add_x=1, extra=1.5, flip=True),
            tri(xs[0], -0.6, 0, tex="synth_albedo"), tri(xs[1], -0.6, 3, rtex="synth_rough"), tri(xs[2], -0.6, 0, checker=1), tri(xs[3], -0.6, 5),
            tri(xs[4], -0.6, 0, add_x=1, tex="synth_albedo", rtex="synth_rough", tc=[[-1.3, 2.2], [0.4, -0.7], [3.1, 0.5]]),
            # a floor under everything: scattered rays come back into the scene instead of leaving it at the first bounce
            {"type": 2, "v0": [-3.0, -3.0, -0.3], "v1": [3.0, -3.0, -0.3], "v2": [0.0, 4.0, -0.3], "col": [0.7, 0.7, 0.7], "extra": 0.3, "add_x": 0, "mat": 0,
             "norm": None, "vn": None, "smooth": 0, "checker": 1, "tex": "no", "rtex": "no", "tc": None}]


@pytest.fixture(scope="module")
def scenes(tmp_path_factory, synth):
    """background -> (path of the .rts, texture directory): the same objects under both settings lines"""
    d = str(tmp_path_factory.mktemp("phase_arms"))
    out = {}
    for bg in BACKGROUNDS:
        path = os.path.join(d, "arms_%s.rts" % bg)
        with open(path, "w") as f:
            f.write("*,0.5,-3.0,2.0,0.01,0,0,0,4,45,10,1,1,%s,64,64\n" % bg + shade_cases.rts_text(_objects()))
        out[bg] = (path, synth["tex"])
    return out


# the issue's list of arms as predicates on the oracle's object records (orc.OBJ_DTYPE: tex is the checker flag, addional.x is add_x)
_diffuse = lambda o: o["mat"] == 0 and o["texnum"] < 0 and o["rtexnum"] < 0 and o["tex"] == 0
ARMS = {"diffuse without add_x": lambda o: _diffuse(o) and o["addional"][0] == 0, "diffuse with add_x": lambda o: _diffuse(o) and o["addional"][0] != 0,
        "emissive": lambda o: o["mat"] == 1, "mirror": lambda o: o["mat"] == 2, "metal": lambda o: o["mat"] == 3, "glass": lambda o: o["mat"] == 4,
        "glossy": lambda o: o["mat"] == 5, "an unknown material": lambda o: o["mat"] == 7,
        "a textured triangle": lambda o: o["type"] == 2 and o["texnum"] >= 0 and o["rtexnum"] < 0,
        "a roughness texture": lambda o: o["type"] == 2 and o["rtexnum"] >= 0 and o["texnum"] < 0,
        "both textures": lambda o: o["type"] == 2 and o["rtexnum"] >= 0 and o["texnum"] >= 0,
        "the checker flag": lambda o: o["type"] == 2 and o["tex"] != 0 and o["texnum"] < 0,
        "a sphere": lambda o: o["type"] == 0, "a triangle": lambda o: o["type"] == 2,
        "a glass triangle": lambda o: o["type"] == 2 and o["mat"] == 4, "a glass sphere": lambda o: o["type"] == 0 and o["mat"] == 4}


class HitLog:
    """An oracle scene as oracle_radiance sees it (kat_hit, kat_miss, kat_bounce), which keeps the object index of every hit: calls[k] holds the
    objects hit by the (k + 1)-th ray of the paths still alive"""
    def __init__(self, scene):
        self.scene, self.calls = scene, []

    def kat_hit(self, o, d):
        t, idx = self.scene.kat_hit(o, d)
        self.calls.append(np.array(idx[t > 0], np.int64))
        return t, idx

    def kat_miss(self, *a):
        return self.scene.kat_miss(*a)

    def kat_bounce(self, *a):
        return self.scene.kat_bounce(*a)


@pytest.fixture(scope="module")
def oracle(scenes):
    """background -> the oracle's side, computed once before the process touches the GPU: settings, the sum of the launch's frames, and the branches
    the paths of its first frame take"""
    from oracle import orc
    out = {}
    for bg in BACKGROUNDS:
        path, tex = scenes[bg]
        o = radiance_cases.oracle_scene(path, tex)
        s = o.settings()
        st = orc.settings13(s, 1, spp=1)
        frames = sum(o.render(st, W, H, s.background, SEED + STRIDE * k, nthreads=8)[0].astype(np.int64) for k in range(FRAMES))
        x, y = (a.ravel().astype(np.int32) for a in np.meshgrid(np.arange(W), np.arange(H), indexing="ij"))
        ro, rd, nx = orc.kat_camera(st, W, H, SEED, W, x, y, np.zeros_like(x))
        seeds = (np.uint64(SEED) + x.astype(np.uint64) + y.astype(np.uint64) * np.uint64(W))
        words = np.stack([orc.kat_rng_u32(int(v), radiance_cases.M_WORDS) for v in seeds])
        skip = radiance_cases.position_after(words, nx, np.zeros(len(x), np.int32))
        log = HitLog(o)
        paths = radiance_cases.oracle_radiance(log, ro, rd, 1, int(st[9]), s.background, int(st[12]), seeds=seeds, skip=skip)
        out[bg] = {"st": st, "bg": s.background, "frames": frames, "paths": paths, "backtex": int(st[12]), "hits": log.calls, "objects": o.objects()}
        o.close()
    return out


@pytest.mark.parametrize("bg", BACKGROUNDS)
def test_every_arm_is_taken_on_the_oracles_side(oracle, bg):
    from oracle import orc
    e = oracle[bg]
    assert int(e["st"][9]) == 10 and (e["backtex"] >= 0) == (bg != "no")
    taken = dict(zip(orc.BRANCHES, (int(v) for v in e["paths"]["branches"])))
    print(bg, taken, "first rays that miss", e["paths"]["first_miss"], "paths at the depth limit", e["paths"]["exhausted"])
    assert all(v > 0 for v in taken.values()), taken
    # shade_material's own arms, and the two that share one branch: which OBJECTS the paths hit, by the oracle's records of them (kat_hit's index)
    ob = e["objects"][:len(_objects())]
    assert len(e["objects"]) == len(_objects()) + 1
    camera, scattered = set(e["hits"][0].tolist()), set(np.concatenate(e["hits"][1:]).tolist())
    print(bg, "objects hit by camera rays", sorted(camera), "by later rays", sorted(scattered))
    assert camera == set(range(len(ob))) and scattered == set(range(len(ob))), "an object of the scene is hit by no camera ray, or by no scattered ray"
    for name, has in ARMS.items():
        idx = {k for k, o in enumerate(ob) if has(o)}
        assert idx and idx & camera and idx & scattered, name
    assert e["paths"]["first_miss"] > 0 and e["paths"]["exhausted"] > 0, (e["paths"]["first_miss"], e["paths"]["exhausted"])


@pytest.mark.parametrize("bg", BACKGROUNDS)
def test_the_lean_build_equals_the_oracle(oracle, scenes, bg):
    e = oracle[bg]                         # (the oracle first)
    import dogeray_amd as dr
    assert dr.device_count() >= 1, "no GPU visible: the HIP path cannot run (there is no fallback)"
    sc = dr.Scene.load(scenes[bg][0], scenes[bg][1]); sc.build_bvh()
    st = dr.pack_settings13(sc.settings(), 1, spp=1)
    assert np.array_equal(np.asarray(st, np.float32), e["st"])
    c = dr.Context(0)
    try:
        c.set_option("coop_steps", 0); c.set_option("occupancy", 6); c.set_option("sample_order", 1); c.set_option("batch_frames", FRAMES)
        c.upload(sc)
        c.stats_reset()
        c.accum_reset(W, H)
        c.render_accumulate(st, W, H, e["bg"], SEED, STRIDE, FRAMES)
        assert c.stats()["launches"] == 1
        got = c.accum_read().astype(np.int64)
    finally:
        c.close()
    assert np.array_equal(got, e["frames"]), "%d pixels differ" % int((got != e["frames"]).any(axis=2).sum())
