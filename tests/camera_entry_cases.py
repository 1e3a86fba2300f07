"""The scenes and views of the camera rays' entry table's tests (option camera_entry), shared by the host and the GPU test: every
scene of tests/ray_cases.py, hf_small at scales 1 and 0.1 (and 0.02 for the GPU: scaled down, its triangles enter the wide tree with their own
bounds and the view has a grazing certificate, which the device's table lives beside), bunny_small, matball (spheres) and the cube; each from its
own camera, the height fields from straight above as well; the lens closed, the scene's own, and 20 times that."""
import os

import numpy as np

import cert_level_cases
import ray_cases
from conftest import CUBE_SETTINGS, SCENES as GOLDEN_SCENES, with_settings

SIZES = ((64, 40), (72, 44))      # 8 x 5 tiles; 9 x 5 tiles with four pixels of margin on either axis
SEED, STRIDE, FRAMES = 5, 1000003, 8
NAMED = ("hf_1", "hf_0.1", "bunny_small", "matball", "cube")
HF_SCALE = {"hf_1": 1.0, "hf_0.1": 0.1, "hf_0.02": 0.02}


def scaled_rts(src, dst, k):
    """a copy of a scene of triangles with every position (vertices, camera, look-at, focus distance) times k"""
    out = []
    for line in open(src).read().split("\n"):
        c = line.split(",")
        if line.startswith("*"):
            for i in (1, 2, 3, 5, 6, 7, 8):
                c[i] = repr(float(c[i]) * k)
        elif len(c) > 15 and c[3].strip() == "2":
            for i in (0, 1, 2, 9, 10, 11, 13, 14, 15):
                c[i] = repr(float(c[i]) * k)
        out.append(",".join(c))
    open(dst, "w").write("\n".join(out))
    return dst


def paths(synth, d):
    """name -> (.rts, texture directory)"""
    d = str(d)
    out = {}
    for make in ray_cases.SCENES.values():
        for p in make(d):
            out[os.path.splitext(os.path.basename(p))[0]] = (p, "")
    hf = os.path.join(synth["dir"], "hf_small.rts")
    out["hf_1"] = (hf, "")
    out["hf_0.1"] = (scaled_rts(hf, os.path.join(d, "hf_0.1.rts"), 0.1), "")
    out["hf_0.02"] = (scaled_rts(hf, os.path.join(d, "hf_0.02.rts"), 0.02), "")
    out["bunny_small"] = (os.path.join(synth["dir"], "bunny_small.rts"), "")
    out["matball"] = (os.path.join(synth["dir"], "matball.rts"), synth["tex"])
    out["cube"] = (with_settings(os.path.join(GOLDEN_SCENES, "cube.rts"), os.path.join(d, "cube.rts"), CUBE_SETTINGS), "")
    return out


def lens(st, k):
    """the view with the lens radius 0, the scene's own, or 20 times that (a scene with a pinhole: 0.002 of its focus distance, and 20 times that)"""
    out = np.array(st, np.float32).copy()
    own = out[6] if out[6] > 0 else np.float32(0.002) * out[7]
    out[6] = (np.float32(0), own, np.float32(20) * own)[k]
    return out


def views(name, st):
    """the scene's own view; a height field also from straight above (cert_level_cases' "top")"""
    return [np.array(st, np.float32)] + ([cert_level_cases.view(st, "top", HF_SCALE[name])] if name in HF_SCALE else [])


def top(name, st):
    return cert_level_cases.view(st, "top", HF_SCALE[name])


def _small_tri(c, h=0.05):
    return ray_cases.tri_line((c[0] - h, c[1], c[2] - h), (c[0] + h, c[1], c[2] - h), (c[0], c[1], c[2] + h))


def one_triangle_scene(d):
    """a triangle far smaller than a tile straight ahead of ray_cases' camera, and two more far off to the side (a tree needs two leaves)"""
    return ray_cases._write(os.path.join(str(d), "one.rts"), [_small_tri((0.0, 0.0, 0.0)), _small_tri((40.0, 30.0, 0.0)), _small_tri((41.0, 30.0, 0.0))])


def pair_scene(d):
    """two such triangles side by side in one tile -- leaves of consecutive ranks --, and the two far ones"""
    return ray_cases._write(os.path.join(str(d), "pair.rts"), [_small_tri((-0.08, 0.0, 0.0)), _small_tri((0.08, 0.0, 0.0)), _small_tri((40.0, 30.0, 0.0)),
                                                               _small_tri((41.0, 30.0, 0.0))])
