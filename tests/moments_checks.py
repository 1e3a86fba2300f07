"""A numpy int64 / uint64 / float64 restatement of the second-moment plane (include/dogeray_amd.h "second moments",
dogeray_amd/csrc/device_moments.hpp), in the same operation order, over whole planes at once: the fused add, the carry across a reprojection,
the noise estimate of dr_accum_error and the denoiser's temporal variance.  Shared by tests/test_moments_host.py and tests/test_gpu_moments.py."""
import numpy as np

import denoise_checks as dc

CAP = 1 << 26
U64_MAX = np.uint64(2 ** 64 - 1)
THRESHOLDS = np.array([2.0 ** k for k in range(-6, 9)], np.float32)      # bin k (k >= 1) starts at 2^(k-7)


def luma(rgb):
    """(54 r + 183 g) + 19 b in int64 for int32[..., 3]"""
    a = np.asarray(rgb).astype(np.int64)
    return (54 * a[..., 0] + 183 * a[..., 1]) + 19 * a[..., 2]


def square(frame):
    """what one frame adds to M2: the capped luma, squared, as uint64"""
    yc = np.clip(luma(frame), -CAP, CAP)
    return (yc * yc).astype(np.uint64)


def sat_add(m2, sq):
    with np.errstate(over="ignore"):
        s = m2 + sq
    return np.where(s < m2, U64_MAX, s).astype(np.uint64)


def add(acc, m2, frame):
    """(acc + frame, M2 + yc^2 saturating) for acc / frame int32[W, H, 3], m2 uint64[W, H]"""
    frame = np.asarray(frame, np.int32)
    with np.errstate(over="ignore"):
        acc2 = (np.asarray(acc, np.int32) + frame).astype(np.int32)
    return acc2, sat_add(np.asarray(m2, np.uint64), square(frame))


def capped(frame):
    return np.abs(luma(frame)) > CAP


def carry(m2, cnt, max_history):
    """M2 of a valid pixel that carries cnt samples: as it is up to max_history, beyond that (M2 / cnt) * mh + ((M2 % cnt) * mh) / cnt"""
    m2 = np.asarray(m2, np.uint64)
    c = np.maximum(np.asarray(cnt, np.int64), 1).astype(np.uint64)
    mh = np.uint64(max_history)
    scaled = (m2 // c) * mh + ((m2 % c) * mh) // c
    return np.where(np.asarray(cnt, np.int64) <= max_history, m2, scaled).astype(np.uint64)


def variance(acc, m2, n):
    """(estimated, var_p float64) per pixel: acc int32[..., 3], m2 uint64[...], n int64[...]"""
    n = np.asarray(n, np.int64)
    est = n >= 2
    nn = np.where(est, n, 2).astype(np.float64)
    S1d = luma(acc).astype(np.float64)
    M2d = np.asarray(m2, np.uint64).astype(np.float64)
    ss = M2d - (S1d * S1d) / nn
    ss = np.where(ss > 0, ss, 0.0)
    var = (ss / ((nn - 1.0) * nn)) / 65536.0
    return est, np.where(est, var, 0.0)


def error(acc, hist, m2, gw, gh, divide_by, tolerance):
    """dr_accum_error: acc int32[W, H, 3], hist int32[W, H] or None, m2 uint64[W, H] -> (sigma float32[H, W], result dict)"""
    acc = np.asarray(acc, np.int32)
    W, H = acc.shape[0], acc.shape[1]
    h = np.zeros((gw, gh), np.int64) if hist is None else np.asarray(hist)[:gw, :gh].astype(np.int64)
    est, var = variance(acc[:gw, :gh], np.asarray(m2)[:gw, :gh], h + int(divide_by))
    sig = np.where(est, np.sqrt(var), 0.0).astype(np.float32)
    sigma = np.zeros((H, W), np.float32)
    sigma[:gh, :gw] = sig.T
    q = var * 65536.0
    q16 = np.where(q < float(2 ** 40), np.floor(np.minimum(q, float(2 ** 40))), float(2 ** 40)).astype(np.uint64)
    bins = (sig[..., None] >= THRESHOLDS).sum(axis=-1)
    res = {"pixels": gw * gh, "estimated": int(est.sum()), "above": int((est & (sig > np.float32(tolerance))).sum()),
           "sum_var_q16": sum(int(v) for v in q16[est]), "bins": [int(((bins == k) & est).sum()) for k in range(16)]}
    return sigma, res


def denoise(acc, settings13, divide_by, normal, albedo, depth, material, m2=None, hist=None, **params):
    """dr_accum_denoise with option "denoise_variance" = 1 (m2 given): denoise_checks.denoise with the variance of pixels with n >= 4 samples and
    la != 0 taken from the plane.  m2 None: the spatial estimate everywhere."""
    f32 = np.float32
    p = dict(dc.DEFAULTS)
    p.update(params)
    acc = np.asarray(acc, dtype=np.int32)
    W, H = acc.shape[0], acc.shape[1]
    gw, gh = dc.grid(settings13, W, H)
    out = np.zeros((H, W, 3), np.float32)
    with np.errstate(all="ignore"):
        n = np.full((gh, gw), int(divide_by), np.int64) if hist is None else (np.asarray(hist)[:gw, :gh].T.astype(np.int64) + int(divide_by))
        a = np.ascontiguousarray(acc[:gw, :gh].transpose(1, 0, 2))
        c = np.where(n[..., None] == 0, f32(0), a.astype(np.float32) / n.astype(np.float32)[..., None]).astype(np.float32)
        assert p["iterations"] > 0
        m = np.asarray(material, np.int32)
        z = np.asarray(depth, np.float32)
        nz = np.concatenate([np.asarray(normal, np.float32), z[..., None]], axis=2)
        ap = dc.albedo_prime(np.asarray(albedo, np.float32), m, p["demodulate"])
        gz = dc.gradient(z, m)
        e = (c / ap).astype(np.float32)
        var = dc.variance(p, nz, m, gz, dc.lum(e))
        temporal = np.zeros((gh, gw), bool)
        if m2 is not None:
            la = dc.lum(ap)
            _, vp = variance(a, np.asarray(m2)[:gw, :gh].T, np.maximum(n, 2))
            temporal = (n >= 4) & (la != f32(0))
            var = np.where(temporal, (vp / (la.astype(np.float64) * la.astype(np.float64))).astype(np.float32), var)
        for i in range(p["iterations"]):
            e, var = dc.atrous(p, nz, m, gz, e, var, 1 << i)
        out[:gh, :gw] = (e * ap).astype(np.float32)
        rgb = np.fmin(np.fmax(out, f32(0)), f32(255)).astype(np.int32).astype(np.uint8)
    return out, rgb, temporal
