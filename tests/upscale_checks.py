"""A numpy float32 restatement of the AOV-guided upsampler (include/dogeray_amd.h dr_accum_upscale, dogeray_amd/csrc/device_upscale.hpp), in
the same operation order, over the whole output grid at once: a tap that is skipped leaves the sums as they were (np.where), so the image
equals the device functions' bit for bit.  The low side (colour, demodulation, the optional a-trous prefilter) is denoise_checks'.  Shared by
tests/test_upscale_host.py and tests/test_gpu_upscale.py."""
import numpy as np

import denoise_checks as dc

f32 = np.float32
MISS = dc.MISS
BLOCK, GUIDED = 0, 1
DEFAULTS = {"mode": GUIDED, "normal_power_log2": 5, "sigma_depth": 1.0, "demodulate": 1, "material_stop": 1}


def low_colour(acc, hist, gw, gh, divide_by):
    """c of the low grid, [gh, gw, 3]"""
    a = np.ascontiguousarray(acc[:gw, :gh].transpose(1, 0, 2)).astype(np.float32)
    if hist is None:
        return (a / f32(divide_by)).astype(np.float32)
    n = (np.asarray(hist)[:gw, :gh].T.astype(np.int64) + int(divide_by)).astype(np.float32)[..., None]
    return np.where(n == 0, f32(0), a / n).astype(np.float32)


def present8(acc, hist, gw, gh, divide_by):
    """dr_accum_present's integer image of the low grid, [gh, gw, 3]"""
    a = acc[:gw, :gh].transpose(1, 0, 2).astype(np.int64)
    n = np.full((gh, gw, 1), int(divide_by), np.int64)
    if hist is not None:
        n = n + np.asarray(hist)[:gw, :gh].T.astype(np.int64)[..., None]
    v = np.where(n == 0, 0, np.trunc(a / np.where(n == 0, 1, n)))
    return np.clip(v, 0, 255).astype(np.uint8)


def position(n_out, div):
    """(x0 int[n_out], f float32[n_out]) for X = 0 .. n_out - 1"""
    t = 2 * np.arange(n_out, dtype=np.int64) + 1 - div
    x0 = np.floor_divide(t, 2 * div)
    r = t - 2 * div * x0
    return x0, r.astype(np.float32) / f32(2 * div)


def upscale(acc, settings13, divide_by, low_guides, full_guides, hist=None, prefilter=None, **params):
    """The restatement: acc int32[W, H, 3] (column-major, as dr_accum_read), the guides of settings13 (low_guides) and of settings13 with
    element 11 = 1 (full_guides) as Context.render_aov returns them -> (f32[H, W, 3], uint8[H, W, 3], no-tap mask bool[H, W]) in
    dr_accum_present's layout.  prefilter: None or a dict of dr_denoise_params fields; params: the fields of dr_upscale_params; any other name
    is a TypeError."""
    p = dict(DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError("unknown upscale parameter %r" % k)
        p[k] = v
    acc = np.asarray(acc, dtype=np.int32)
    W, H = acc.shape[0], acc.shape[1]
    div = int(f32(settings13[11]))
    gw, gh = dc.grid(settings13, W, H)
    Gw, Gh = gw * div, gh * div
    out = np.zeros((H, W, 3), np.float32)
    rgb = np.zeros((H, W, 3), np.uint8)
    notap = np.zeros((H, W), bool)
    if gw == 0 or gh == 0:
        return out, rgb, notap
    with np.errstate(all="ignore"):
        c = low_colour(acc, hist, gw, gh, divide_by)
        block = np.repeat(np.repeat(c, div, axis=0), div, axis=1)
        if p["mode"] == BLOCK:
            out[:Gh, :Gw] = block
            rgb[:Gh, :Gw] = np.repeat(np.repeat(present8(acc, hist, gw, gh, divide_by), div, axis=0), div, axis=1)
            return out, rgb, notap
        m = np.asarray(low_guides["material"], np.int32)
        z = np.asarray(low_guides["depth"], np.float32)
        nz = np.concatenate([np.asarray(low_guides["normal"], np.float32), z[..., None]], axis=2)
        ap = dc.albedo_prime(np.asarray(low_guides["albedo"], np.float32), m, p["demodulate"])
        e = (c / ap).astype(np.float32)
        if prefilter is not None:
            d = dict(dc.DEFAULTS)
            d.update(prefilter)
            assert d["iterations"] >= 1 and bool(d["demodulate"]) == bool(p["demodulate"])
            gz = dc.gradient(z, m)
            var = dc.variance(d, nz, m, gz, dc.lum(e))
            for i in range(d["iterations"]):
                e, var = dc.atrous(d, nz, m, gz, e, var, 1 << i)
        M = np.asarray(full_guides["material"], np.int32)
        Z = np.asarray(full_guides["depth"], np.float32)
        GZ = dc.gradient(Z, M)[:Gh, :Gw]
        AP = dc.albedo_prime(np.asarray(full_guides["albedo"], np.float32), M, p["demodulate"])[:Gh, :Gw]
        N = np.asarray(full_guides["normal"], np.float32)[:Gh, :Gw]
        M, Z = M[:Gh, :Gw], Z[:Gh, :Gw]
        x0, fx = position(Gw, div)
        y0, fy = position(Gh, div)
        bx = [f32(1) - fx, fx]
        by = [f32(1) - fy, fy]
        rz = f32(1) / ((f32(p["sigma_depth"]) * GZ) * f32(div) + f32(1e-3) * Z)
        sw = np.zeros((Gh, Gw), np.float32)
        s = np.zeros((Gh, Gw, 3), np.float32)
        for j in range(2):
            for i in range(2):
                qx, qy = x0 + i, y0 + j
                inside = ((qx >= 0) & (qx < gw))[None, :] & ((qy >= 0) & (qy < gh))[:, None]
                ix, iy = np.clip(qx, 0, gw - 1)[None, :], np.clip(qy, 0, gh - 1)[:, None]
                mq, nq, eq = m[iy, ix], nz[iy, ix], e[iy, ix]
                b = (bx[i][None, :] * by[j][:, None]).astype(np.float32)
                ok = inside & (b != f32(0)) & ((M == MISS) == (mq == MISS))
                if p["material_stop"]:
                    ok &= M == mq
                wn = np.fmax((N[..., 0] * nq[..., 0] + N[..., 1] * nq[..., 1]) + N[..., 2] * nq[..., 2], f32(0))
                for _ in range(p["normal_power_log2"]):
                    wn = wn * wn
                dz = np.abs(Z - nq[..., 3])
                xz = np.where(dz > f32(0), dz * rz, f32(0))
                w = np.where(M == MISS, b, (b * wn) / dc.q(xz)).astype(np.float32)
                sw = np.where(ok, sw + w, sw)
                s = np.where(ok[..., None], s + w[..., None] * eq, s)
        found = sw > f32(0)
        f = np.where(found[..., None], (s / sw[..., None]) * AP, block).astype(np.float32)
        out[:Gh, :Gw] = f
        notap[:Gh, :Gw] = ~found
        rgb = np.fmin(np.fmax(out, f32(0)), f32(255)).astype(np.int32).astype(np.uint8)
    return out, rgb, notap
