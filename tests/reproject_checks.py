"""A numpy float64 / int64 restatement of the temporal reprojection (include/dogeray_amd.h dr_accum_reproject,
dogeray_amd/csrc/device_reproject.hpp), written from the header's text in the same operation order, over whole planes at once, so that its
planes and counts equal the device functions' bit for bit.  A view's float camera block (from, llc, hor, ver, den_w, den_h as dr_render_frame
forms them) is an input: tools/host_kernel.py camera_block hands it out, and directions() is checked against dr_render_aov's `dir` channel.
Shared by tests/test_reproject_host.py and tests/test_gpu_reproject.py."""
import numpy as np

f32, f64, i64 = np.float32, np.float64, np.int64
DEFAULTS = {"max_history": 32, "normal_cos": 0.9, "plane_tolerance": 0.01, "material_mask": 0xFFFFFFC3, "sky": 1}
CLASSES = ("valid", "masked", "offscreen", "rejected")


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def directions(cam, x, y):
    """d(view, x, y): float32 [..., 3] for integer arrays x, y"""
    nu = ((x.astype(f64) + 0.5) / f64(cam["den_w"])).astype(f32)
    nv = ((y.astype(f64) + 0.5) / f64(cam["den_h"])).astype(f32)
    frm, llc, hor, ver = (np.asarray(cam[k], f32) for k in ("from", "llc", "hor", "ver"))
    return ((llc + nu[..., None] * hor) + nv[..., None] * ver) - frm


def projection(cam):
    """(L, cN, L . cN, hor, ver, hor . hor, ver . ver) of the `from` camera in float64, or None for a degenerate view"""
    frm, llc, hor, ver = (np.asarray(cam[k], f32).astype(f64) for k in ("from", "llc", "hor", "ver"))
    L = llc - frm
    cN = np.array([hor[1] * ver[2] - hor[2] * ver[1], hor[2] * ver[0] - hor[0] * ver[2], hor[0] * ver[1] - hor[1] * ver[0]])
    if dot(cN, L) < 0:
        cN = -cN
    LcN = dot(L, cN)
    if not np.isfinite(LcN) or LcN == 0:
        return None
    return L, cN, LcN, hor, ver, dot(hor, hor), dot(ver, ver)


def allowed(m, p):
    """material m (int array) carried?  a miss by `sky`, a hit by bit m (0 .. 30) or bit 31 (every other id) of material_mask"""
    bit = np.where((m < 0) | (m > 31), 31, m).astype(np.uint64)
    hit_ok = ((np.uint64(p["material_mask"] & 0xFFFFFFFF) >> bit) & np.uint64(1)) != 0
    return np.where(m == -1, bool(p["sky"]), hit_ok)


def reproject(acc, hist, frames, cam_from, cam_to, guides_from, guides_to, gw, gh, **params):
    """acc int32[W, H, 3] (column-major as dr_accum_read returns it), hist int32[W, H] or None; guides: dicts with "t" [gh, gw], "normal"
    [gh, gw, 3], "material" [gh, gw] -> (acc_to, hist_to, counts, info); info: "cls" [gh, gw] (index into CLASSES), "qx", "qy" (of the pixels
    that project into the grid) and "behind", the number of unmasked pixels whose world point is not in front of the `from` camera"""
    p = dict(DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError("unknown reproject parameter %r" % k)
        p[k] = v
    if not (1 <= p["max_history"] <= 65535) or not (-1 <= f32(p["normal_cos"]) <= 1) or not (f32(p["plane_tolerance"]) >= 0) or frames < 1:
        raise ValueError("bad reproject parameters")
    J = projection(cam_from)
    if J is None:
        raise ValueError("degenerate from view")
    L, cN, LcN, hor, ver, hh, vv = J
    W, H = acc.shape[0], acc.shape[1]
    y, x = np.meshgrid(np.arange(gh), np.arange(gw), indexing="ij")
    mp = np.asarray(guides_to["material"], np.int32)
    miss = mp == -1
    with np.errstate(all="ignore"):
        d = directions(cam_to, x, y).astype(f64)
        tp = np.asarray(guides_to["t"], f32).astype(f64)
        X = np.asarray(cam_to["from"], f32).astype(f64) + tp[..., None] * d
        v = np.where(miss[..., None], d, X - np.asarray(cam_from["from"], f32).astype(f64))
        a = dot(v, cN)
        s = LcN / a
        r = s[..., None] * v - L
        nu, nv = dot(r, hor) / hh, dot(r, ver) / vv
        fx, fy = np.floor(nu * f64(cam_from["den_w"])), np.floor(nv * f64(cam_from["den_h"]))
        masked = ~allowed(mp, p)
        inside = (a > 0) & (fx >= 0) & (fx < gw) & (fy >= 0) & (fy < gh)
        offscreen = ~masked & ~inside
        live = ~masked & inside
        qx = np.where(live, fx, 0).astype(np.int64)
        qy = np.where(live, fy, 0).astype(np.int64)
        mq = np.asarray(guides_from["material"], np.int32)[qy, qx]
        n_p = np.asarray(guides_to["normal"], f32).astype(f64)
        n_q = np.asarray(guides_from["normal"], f32).astype(f64)[qy, qx]
        dq = directions(cam_from, qx, qy).astype(f64)
        tq = np.asarray(guides_from["t"], f32).astype(f64)[qy, qx]
        e = X - (np.asarray(cam_from["from"], f32).astype(f64) + tq[..., None] * dq)
        off = dot(e, n_p)
        dist = np.where(off < 0, -off, off)
        same_surface = (dot(n_p, n_q) >= f64(f32(p["normal_cos"]))) & (dist <= f64(f32(p["plane_tolerance"])) * np.sqrt(dot(v, v)))
    valid = live & (mq == mp) & (miss | same_surface)
    rejected = live & ~valid
    cls = np.select([masked, offscreen, rejected], [1, 2, 3], 0)
    # the carry
    accq = acc[:gw, :gh].astype(i64)[qx, qy]                       # [gh, gw, 3]
    hq = (hist[:gw, :gh].astype(i64)[qx, qy] if hist is not None else np.zeros((gh, gw), i64))
    cnt = hq + i64(frames)
    mh = i64(p["max_history"])
    prod = accq * mh
    scaled = np.sign(prod) * (np.abs(prod) // np.maximum(cnt, 1)[..., None])      # towards zero
    capped = cnt > mh
    out_acc = np.where(capped[..., None], scaled, accq)
    out_hist = np.where(capped, mh, cnt)
    acc_to = np.zeros((W, H, 3), np.int32)
    hist_to = np.zeros((W, H), np.int32)
    acc_to[:gw, :gh] = np.where(valid[..., None], out_acc, 0).transpose(1, 0, 2).astype(np.int32)
    hist_to[:gw, :gh] = np.where(valid, out_hist, 0).T.astype(np.int32)
    counts = {"pixels": gw * gh}
    for k, name in enumerate(CLASSES):
        counts[name] = int((cls == k).sum())
    return acc_to, hist_to, counts, {"cls": cls, "qx": qx, "qy": qy, "behind": int((~masked & ~(a > 0)).sum())}


def moves(st):
    """Five camera moves away from settings13 st, as settings13: a sideways translation, a dolly, a look-at change, an fov change, and a
    camera that has gone past the look-at point and looks back (much of what it sees lies behind the old camera)"""
    st = np.asarray(st, f32)
    cam, look = st[0:3].astype(f64), st[3:6].astype(f64)
    fwd = look - cam
    dist = np.linalg.norm(fwd)
    right = np.cross(fwd / dist, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd / dist)

    def make(cam2=None, look2=None, fov=None):
        out = st.copy()
        if cam2 is not None:
            out[0:3] = cam2
        if look2 is not None:
            out[3:6] = look2
        if fov is not None:
            out[8] = fov
        return out
    return {"sideways": make(cam + 0.05 * dist * right, look + 0.05 * dist * right),
            "dolly": make(cam + 0.15 * fwd),
            "look": make(look2=look + 0.12 * dist * right + 0.05 * dist * up),
            "fov": make(fov=st[8] - 7),
            "behind": make(cam + 1.6 * fwd)}
