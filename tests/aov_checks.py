"""Independent checks of first-hit AOV buffers (dr_render_aov / the host build's hk_aov), shared by tests/test_aov_host.py and
tests/test_gpu_aov.py: the oracle's kat_hit / kat_normal on the returned rays, and numpy float32 restatements of albedo, distance and
depth.  Every comparison is bitwise, except the ray direction against its float64 restatement."""
import os

import numpy as np

from conftest import CUBE_SETTINGS, SCENES, with_settings

CHANNELS = ("t", "distance", "depth", "object", "material", "normal", "uv", "albedo", "dir")


def scene_cases(synth, tmp_path):
    """(name, .rts path, texture dir, W, H) of the scenes the AOV tests cover; files without a '*' line get the cube's camera."""
    cases = []
    for name in ("cube", "mats", "textest", "uv", "smooth", "norm", "cow"):
        path = os.path.join(SCENES, name + ".rts")
        if not any(l.startswith("*") for l in open(path)):
            path = with_settings(path, str(tmp_path / (name + ".rts")), CUBE_SETTINGS)
        cases.append((name, path, synth["tex"] if name == "cow" else "", 136, 96))
    cases.append(("hf_small", os.path.join(synth["dir"], "hf_small.rts"), "", 160, 96))
    cases.append(("city_small", os.path.join(synth["dir"], "city_small.rts"), "", 160, 96))
    return cases


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def f2i(f):
    """float -> int as cvt.rzi.s32.f32: saturating, NaN -> 0"""
    f = np.asarray(f, dtype=np.float64)
    return np.where(np.isnan(f), 0, np.trunc(np.clip(np.nan_to_num(f), -2147483648.0, 2147483647.0))).astype(np.int64)


def texel_rgb(tex, u, v):
    """tex2D point / wrap / normalised (K:830) and b / 255 for arrays u, v (float32): float32[n, 3]"""
    th, tw = tex.shape[0], tex.shape[1]
    u = u.astype(np.float32)
    v = v.astype(np.float32)
    fu = (u - np.floor(u)).astype(np.float32)
    fv = (v - np.floor(v)).astype(np.float32)
    i = np.clip(f2i(np.floor(fu * np.float32(tw))), 0, tw - 1)
    j = np.clip(f2i(np.floor(fv * np.float32(th))), 0, th - 1)
    px = tex[j, i, :3].astype(np.float32)
    return (px / np.float32(255)).astype(np.float32)


def albedo_numpy(objects, textures, obj, uv):
    """ocolor of K:826-844 for hits on objects obj with texture coordinates uv (float32[n, 2])"""
    o = objects[obj]
    col = o["col"].astype(np.float32)
    out = col.copy()
    ntex = len(textures)
    texnum = np.where((o["texnum"] >= 0) & (o["texnum"] < ntex), o["texnum"], -1)
    u, v = uv[:, 0].astype(np.float32), uv[:, 1].astype(np.float32)
    vt = (-v + np.float32(1)).astype(np.float32)
    for k in range(ntex):
        m = texnum == k
        if m.any():
            out[m] = texel_rgb(textures[k], u[m], vt[m])
    chk = (texnum < 0) & (o["tex"] != 0)
    if chk.any():
        yes = (np.floor(u[chk] * np.float32(10)) + np.floor(v[chk] * np.float32(10))).astype(np.float32)
        even = np.fmod(yes, np.float32(2)) == 0
        out[chk] = np.where(even[:, None], np.float32(0.8), col[chk])
    return out


def pinhole_dirs64(st, W, H, x, y):
    """K:1016-1049 in float64: the direction of the ray through the centre of pixel (x, y)"""
    st = np.asarray(st, dtype=np.float64)
    div = st[11]
    aspect = (W / div) / (H / div)
    vh = 2.0 * np.tan(st[8] * np.pi / 180 / 2)
    vw = aspect * vh
    frm, at = st[0:3], st[3:6]
    w = (frm - at) / np.linalg.norm(frm - at)
    u = np.cross([0.0, 1.0, 0.0], w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    hor, ver = st[7] * vw * u, st[7] * vh * v
    llc = frm - hor / 2 - ver / 2 - st[7] * w
    nu = (np.asarray(x, np.float64) + 0.5) / np.float64(np.float32(W / np.float32(div)))
    nv = (np.asarray(y, np.float64) + 0.5) / np.float64(np.float32(H / np.float32(div)))
    return llc + nu[..., None] * hor + nv[..., None] * ver - frm


def check_against_oracle(aov, orc_scene, st, W, H, window, what=""):
    """The independent checks of one window's channels (dict of numpy arrays, all channels)."""
    x0, y0, w, h = window
    st = np.asarray(st, dtype=np.float32)
    d = aov["dir"].reshape(-1, 3)
    n = d.shape[0]
    o = np.broadcast_to(st[0:3], (n, 3)).astype(np.float32)
    # the direction: the pinhole through the pixel centre
    yy, xx = np.mgrid[y0:y0 + h, x0:x0 + w]
    want = pinhole_dirs64(st, W, H, xx.ravel(), yy.ravel())
    err = np.linalg.norm(d.astype(np.float64) - want, axis=1) / np.linalg.norm(want, axis=1)
    assert err.max() < 1e-6, "%s: dir off by %.3g relative" % (what, err.max())
    # t / object: the oracle's hit() on the same rays
    t_ref, idx_ref = orc_scene.kat_hit(o, d)
    t, obj = aov["t"].ravel(), aov["object"].ravel()
    assert same_bits(t, t_ref), "%s: t differs from the oracle at %d pixels" % (what, int((bits(t) != bits(t_ref)).sum()))
    hit = t > 0
    assert np.array_equal(obj[hit], idx_ref[hit]) and (obj[~hit] == -1).all(), what
    assert hit.any(), "%s: nothing hit" % what
    objects = orc_scene.objects()
    assert np.array_equal(aov["material"].ravel()[hit], objects["mat"][obj[hit]]) and (aov["material"].ravel()[~hit] == -1).all(), what
    # distance / depth
    dh = d[hit]
    t32 = t[hit].astype(np.float32)
    dist = (t32 * np.sqrt((dh[:, 0] * dh[:, 0] + dh[:, 1] * dh[:, 1]) + dh[:, 2] * dh[:, 2]).astype(np.float32)).astype(np.float32)
    assert same_bits(aov["distance"].ravel()[hit], dist), what
    assert same_bits(aov["depth"].ravel()[hit], (t32 * st[7]).astype(np.float32)), what
    assert np.isposinf(aov["distance"].ravel()[~hit]).all() and np.isposinf(aov["depth"].ravel()[~hit]).all(), what
    # normal / uv: the oracle's getnormal, flipped to face the ray
    nrm_ref, tc_ref = orc_scene.kat_normal(obj[hit], o[hit], dh, t32)
    dn = ((dh[:, 0] * nrm_ref[:, 0] + dh[:, 1] * nrm_ref[:, 1]) + dh[:, 2] * nrm_ref[:, 2]).astype(np.float32)
    nrm_ref = np.where((dn < 0)[:, None], nrm_ref, -nrm_ref)
    assert same_bits(aov["normal"].reshape(-1, 3)[hit], nrm_ref), what
    assert same_bits(aov["uv"].reshape(-1, 2)[hit], tc_ref[:, :2]), what
    # albedo: the numpy restatement
    alb = albedo_numpy(objects, orc_scene.textures(), obj[hit], tc_ref[:, :2])
    got = aov["albedo"].reshape(-1, 3)[hit]
    assert same_bits(got, alb), "%s: albedo differs at %d hits" % (what, int((bits(got) != bits(alb)).any(axis=1).sum()))
    for k in ("normal", "uv", "albedo"):
        assert not aov[k].reshape(n, -1)[~hit].any(), what
    return int(hit.sum())
