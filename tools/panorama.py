"""A 360-degree equirectangular image of a scene, a camera the pinhole path cannot do:   python tools/panorama.py scene.rts out.pfm [width=1024] [passes=16] [texdir]
The rays are made here in numpy -- column x is the longitude, row y the latitude, both jittered inside the pixel per pass, from the scene's camera position
with the scene's view direction in the middle of the image -- and every pass is one Context.radiance call; the passes' float mean goes into a .pfm."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import dogeray_amd as dr


def panorama_rays(eye, look, width, height, rng):
    """(origin, dir) float32 [height * width, 3], row-major: longitude -pi .. pi left to right around the world's up axis (y) with `look` at 0, latitude
    pi/2 .. -pi/2 top to bottom"""
    x, y = np.meshgrid(np.arange(width), np.arange(height))
    lon = ((x + rng.uniform(size=x.shape)) / width - 0.5) * 2.0 * np.pi
    lat = (0.5 - (y + rng.uniform(size=y.shape)) / height) * np.pi
    f = np.array([look[0] - eye[0], 0.0, look[2] - eye[2]])
    f = f / np.linalg.norm(f) if np.linalg.norm(f) > 0 else np.array([0.0, 0.0, -1.0])
    r = np.array([-f[2], 0.0, f[0]])                               # f turned a quarter to the right, seen from above
    d = (np.cos(lat) * np.cos(lon))[..., None] * f + (np.cos(lat) * np.sin(lon))[..., None] * r + np.sin(lat)[..., None] * np.array([0.0, 1.0, 0.0])
    d = d.reshape(-1, 3).astype(np.float32)
    return np.tile(np.asarray(eye, np.float32), (len(d), 1)), d


def render(ctx, settings, width, passes, seed=1):
    height = width // 2
    rng = np.random.default_rng(seed)
    mean = np.zeros((height * width, 3), np.float64)
    for k in range(passes):
        o, d = panorama_rays(settings.campos, settings.look, width, height, rng)
        mean += ctx.radiance(o, d, 1, settings.max_depth, settings.background, settings.backtex, seed=seed + k * 1000003 * width * height)["radiance"]
    return (mean / passes).astype(np.float32).reshape(height, width, 3)


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    width = int(sys.argv[3]) if len(sys.argv) > 3 else 1024
    passes = int(sys.argv[4]) if len(sys.argv) > 4 else 16
    scene = dr.Scene.load(sys.argv[1], sys.argv[5] if len(sys.argv) > 5 else "")
    scene.build_bvh()
    ctx = dr.Context(0).upload(scene)
    img = render(ctx, scene.settings(), width, passes)
    dr.write_pfm(sys.argv[2], img)
    print("%s: %d x %d, %d passes, mean radiance %s" % (sys.argv[2], width, width // 2, passes, img.reshape(-1, 3).mean(axis=0).round(4).tolist()))
    ctx.close()
