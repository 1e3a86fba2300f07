"""The definition of the lens-averaged AOVs (dr_render_aov_lens / the host build's hk_aov_lens) written out in numpy float32, shared by
tests/test_aov_lens_host.py and tests/test_gpu_aov_lens.py: a fold, sample by sample, of the camera rays (dr_kat_camera / hk_kat_camera) through
the closest hit and its surface channels (dr_trace_rays / hk_trace), with the sums, the Boyer-Moore vote and the divisions as
include/dogeray_amd.h writes them.  Every comparison is of bit patterns."""
import os

import numpy as np

from conftest import CUBE_SETTINGS, SCENES, with_settings

CHANNELS = ("coverage", "depth", "distance", "material", "normal", "albedo")
SURFACE = ("t", "material", "distance", "normal", "albedo")
W, H = 72, 56
WINDOW = (3, 5, 50, 37)          # partial tiles on all four sides
SEED, STRIDE = 12345, 1000003
F32 = np.float32


def scene_paths(synth, tmp_path):
    """(name, .rts path) of the scenes the lens tests cover; files without a '*' line get the cube's camera"""
    out = []
    for name in ("cube", "textest"):
        path = os.path.join(SCENES, name + ".rts")
        if not any(l.startswith("*") for l in open(path)):
            path = with_settings(path, str(tmp_path / (name + ".rts")), CUBE_SETTINGS)
        out.append((name, path))
    out.insert(1, ("matball", os.path.join(synth["dir"], "matball.rts")))
    return out


def lens_settings(st, aperture, spp):
    st = np.array(st, dtype=np.float32)
    st[6], st[10] = aperture, spp
    return st


def fold(camera, trace, st, W, H, window, frame_seed, seed_stride, nframes, as_guides=False):
    """camera(settings13, W, H, frame_seed, stride, x, y, sample) -> (origin[2, n, 3], dir[2, n, 3], ..): form 0 is camera_ray's;
    trace(o, d, channels=SURFACE) -> dict.  Returns the dict of CHANNELS over the window (x0, y0, w, h)."""
    st = np.asarray(st, dtype=np.float32)
    x0, y0, w, h = window
    yy, xx = np.mgrid[y0:y0 + h, x0:x0 + w]
    x, y = xx.ravel().astype(np.int32), yy.ravel().astype(np.int32)
    n = x.size
    spp, focus = int(st[10]), F32(st[7])
    stride = 8 * (W // int(st[11]) // 8)                   # the unstriped view's 8 * gx
    N = nframes * spp
    assert 1 <= N <= 256
    hits = np.zeros(n, np.int64)
    depth, distance = np.zeros(n, F32), np.zeros(n, F32)
    normal, albedo = np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    cand, cnt = np.full(n, -1, np.int32), np.zeros(n, np.int64)
    for k in range(nframes):
        seed_k = (int(frame_seed) + k * int(seed_stride)) % 2 ** 64
        for s in range(spp):
            cam = camera(st, W, H, seed_k, stride, x, y, np.full(n, s, np.int32))
            o, d = np.ascontiguousarray(cam[0][0]), np.ascontiguousarray(cam[1][0])
            r = trace(o, d, channels=SURFACE)
            t = r["t"].astype(F32)
            hit = t > 0
            hits += hit
            depth = np.where(hit, depth + (t * focus).astype(F32), depth).astype(F32)
            distance = np.where(hit, distance + np.where(hit, r["distance"], 0).astype(F32), distance).astype(F32)
            normal = np.where(hit[:, None], normal + r["normal"].astype(F32), normal).astype(F32)
            albedo = np.where(hit[:, None], albedo + r["albedo"].astype(F32), albedo).astype(F32)
            v = np.where(hit, r["material"], -1).astype(np.int32)
            assert (r["material"][~hit] == -1).all()
            fresh = cnt == 0                               # the Boyer-Moore vote
            same = ~fresh & (v == cand)
            cand = np.where(fresh, v, cand)
            cnt = np.where(fresh, 1, np.where(same, cnt + 1, cnt - 1))
    hf, nf = hits.astype(F32), F32(N)
    some = hits > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"coverage": (hf / nf).astype(F32),
               "depth": np.where(some, depth / hf, np.inf).astype(F32),
               "distance": np.where(some, distance / hf, np.inf).astype(F32),
               "material": cand.astype(np.int32),
               "normal": np.where(some[:, None], normal / hf[:, None], 0).astype(F32),
               "albedo": (albedo / nf).astype(F32)}
    if as_guides:
        miss = out["material"] == -1
        out["albedo"] = np.where(miss[:, None], 0, out["albedo"] + (F32(1) - out["coverage"])[:, None].astype(F32)).astype(F32)
        out["coverage"] = np.where(miss, 0, out["coverage"]).astype(F32)
        out["depth"] = np.where(miss, np.inf, out["depth"]).astype(F32)
        out["distance"] = np.where(miss, np.inf, out["distance"]).astype(F32)
        out["normal"] = np.where(miss[:, None], 0, out["normal"]).astype(F32)
    return {k: a.reshape((h, w) + a.shape[1:]) for k, a in out.items()}


DEFOCUS = {"campos": (0.0, 1.0, 7.0), "look": (0.0, 1.0, 0.0), "aperture": 0.15, "focus": 3.5, "fov": 40,
           "near": ((-0.9, 0.7, 3.0), 0.7), "far": ((1.3, 1.2, -7.0), 1.2)}


def defocus_scene(dr, path, aperture=None):
    """A checker floor and two spheres of different materials at clearly different depths, the camera focused on the near one: written with
    dogeray_amd.rts_io, 256 x 256.  Returns the path."""
    from dogeray_amd import rts_io
    D = DEFOCUS
    objs = np.zeros(4, dtype=dr.OBJECT_DTYPE)
    objs["texnum"], objs["rtexnum"] = -1, -1
    for o, (c, r), col, mat, rough in ((objs[0], D["near"], (0.85, 0.25, 0.2), 0, 0.0), (objs[1], D["far"], (0.25, 0.45, 0.9), 5, 0.3)):
        o["type"], o["pos"], o["dim"], o["col"], o["mat"], o["addional"] = 0, c, (r, 0, 0), col, mat, (0, rough, 0)
    x0, x1, z0, z1 = -16.0, 16.0, -30.0, 10.0      # the floor y = 0: two triangles, the checker's squares 0.8 wide
    quad = (((x0, 0, z1), (x1, 0, z1), (x1, 0, z0)), ((x0, 0, z1), (x1, 0, z0), (x0, 0, z0)))
    for o, (a, b, c) in zip(objs[2:], quad):
        o["type"], o["pos"], o["dim"], o["rot"], o["norm"], o["col"], o["mat"], o["tex"] = 2, a, b, c, (0, 1, 0), (0.15, 0.15, 0.15), 0, 1
        for k, v in (("t1", a), ("t2", b), ("t3", c)):
            o[k] = ((v[0] - x0) / 8.0, (v[2] - z0) / 8.0, 0)
        for k in ("n1", "n2", "n3"):
            o[k] = (0, 1, 0)
    s = dr.DrSettings()
    s.campos[:], s.look[:] = D["campos"], D["look"]
    s.aperture, s.focus_dist, s.fov, s.max_depth, s.spp = D["aperture"] if aperture is None else aperture, D["focus"], D["fov"], 10, 1
    s.background, s.backtex, s.width, s.height = 1.0, -1, 256, 256
    return rts_io.write_rts(path, objs, s)


def circle_of_confusion(st, W, depth):
    """The diameter, in pixels of a W-wide frame, of the blur of a point at `depth` along the view axis: the lens (diameter st[6]) seen from the point
    spans aperture * |depth - focus| / depth on the focus plane, which is focus * aspect * 2 tan(fov / 2) wide (params_host.hpp fill_view_params)"""
    aperture, focus, fov = float(st[6]), float(st[7]), float(st[8])
    plane = focus * 2.0 * np.tan(np.radians(fov) / 2)          # (aspect 1: the frame is square)
    return aperture * abs(depth - focus) / depth * W / plane


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what, channels=CHANNELS):
    for k in channels:
        g, w = bits(got[k]), bits(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        assert np.array_equal(g, w), "%s: %s differs at %d values" % (what, k, int((g != w).sum()))


def check_properties(a, what):
    """what holds for every output: a material implies a hit, a miss's channels are the miss values"""
    cov = a["coverage"]
    assert ((cov >= 0) & (cov <= 1)).all(), what
    assert (cov[a["material"] != -1] > 0).all(), what
    none = cov == 0
    assert np.isposinf(a["depth"][none]).all() and np.isposinf(a["distance"][none]).all() and (a["material"][none] == -1).all(), what
    assert not a["normal"][none].any() and not a["albedo"][none].any(), what
    assert np.isfinite(a["depth"][~none]).all() and np.isfinite(a["distance"][~none]).all(), what
