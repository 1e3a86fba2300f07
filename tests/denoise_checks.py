"""A numpy float32 restatement of the a-trous denoiser (include/dogeray_amd.h dr_accum_denoise, dogeray_amd/csrc/device_denoise.hpp), in the
same operation order, over whole planes at once: a tap that is skipped leaves the sums as they were (np.where), so the planes equal the device
functions' bit for bit.  Shared by tests/test_denoise_host.py and tests/test_gpu_denoise.py."""
import numpy as np

f32 = np.float32
MISS = -1
OUTSIDE = -2147483648
DEFAULTS = {"iterations": 5, "sigma_luminance": 4.0, "normal_power_log2": 7, "sigma_depth": 1.0, "demodulate": 1, "material_stop": 1}
H5 = [f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625)]
K3 = [f32(0.25), f32(0.5), f32(0.25)]


def grid(settings13, W, H):
    div = int(f32(settings13[11]))
    return W // div // 8 * 8, H // div // 8 * 8


def shift(a, dx, dy, fill):
    """out[y, x] = a[y + dy, x + dx] where that is inside, else fill"""
    out = np.full_like(a, fill)
    gh, gw = a.shape[:2]
    if abs(dx) >= gw or abs(dy) >= gh:
        return out
    out[max(0, -dy):min(gh, gh - dy), max(0, -dx):min(gw, gw - dx)] = a[max(0, dy):min(gh, gh + dy), max(0, dx):min(gw, gw + dx)]
    return out


def q(x):
    return (f32(1) + x) + (f32(0.5) * x) * x


def lum(e):
    return (f32(0.2126) * e[..., 0] + f32(0.7152) * e[..., 1]) + f32(0.0722) * e[..., 2]


def albedo_prime(a, m, demodulate):
    if not demodulate:
        return np.ones_like(a)
    return np.where((m[..., None] == MISS) | (a <= f32(1e-3)), f32(1), a).astype(np.float32)


def gradient(z, m):
    inf = f32(np.inf)
    usable = lambda dx, dy: (shift(m, dx, dy, OUTSIDE) != MISS) & (shift(m, dx, dy, OUTSIDE) != OUTSIDE)
    zr, zl, zd, zu = shift(z, 1, 0, f32(0)), shift(z, -1, 0, f32(0)), shift(z, 0, 1, f32(0)), shift(z, 0, -1, f32(0))
    ar = np.where(usable(1, 0), np.abs(zr - z), inf)
    al = np.where(usable(-1, 0), np.abs(z - zl), inf)
    ad = np.where(usable(0, 1), np.abs(zd - z), inf)
    au = np.where(usable(0, -1), np.abs(z - zu), inf)
    gx, gy = np.fmin(ar, al), np.fmin(ad, au)
    gx = np.where(gx == inf, f32(0), gx)
    gy = np.where(gy == inf, f32(0), gy)
    return np.where(m == MISS, f32(0), np.fmax(gx, gy)).astype(np.float32)


def stop(p, mp, mq):
    ok = (mq != OUTSIDE) & ((mp == MISS) == (mq == MISS))
    if p["material_stop"]:
        ok &= mp == mq
    return ok


def pair(p, nz, m, gz, step, dx, dy):
    """(tap allowed, num, den, the tap's material) of the pair (p, p + step (dx, dy)) for every p"""
    mq = shift(m, step * dx, step * dy, OUTSIDE)
    nq = shift(nz, step * dx, step * dy, f32(0))
    ok = stop(p, m, mq)
    k = abs(dx) + abs(dy)
    if k == 0:
        return ok, np.ones_like(gz), np.ones_like(gz)
    wn = np.fmax((nz[..., 0] * nq[..., 0] + nz[..., 1] * nq[..., 1]) + nz[..., 2] * nq[..., 2], f32(0))
    for _ in range(p["normal_power_log2"]):
        wn = wn * wn
    rz = f32(1) / ((f32(p["sigma_depth"]) * gz) * f32(step * k) + f32(1e-3) * nz[..., 3])
    dz = np.abs(nz[..., 3] - nq[..., 3])
    xz = np.where(dz > f32(0), dz * rz, f32(0))
    hit = m != MISS
    num = np.where(hit, wn, f32(1)).astype(np.float32)
    den = np.where(hit, q(xz), f32(1)).astype(np.float32)
    return ok, num, den


def variance(p, nz, m, gz, l):
    sw = np.zeros_like(gz); s1 = np.zeros_like(gz); s2 = np.zeros_like(gz)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ok, num, den = pair(p, nz, m, gz, 1, dx, dy)
            lq = shift(l, dx, dy, f32(0))
            w = num / den
            sw = np.where(ok, sw + w, sw)
            s1 = np.where(ok, s1 + w * lq, s1)
            s2 = np.where(ok, s2 + w * (lq * lq), s2)
    mu1, mu2 = s1 / sw, s2 / sw
    return np.fmax(mu2 - mu1 * mu1, f32(0))


def atrous(p, nz, m, gz, e, var, step):
    gs = np.zeros_like(gz); gv = np.zeros_like(gz)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            ok = stop(p, m, shift(m, step * dx, step * dy, OUTSIDE))
            kk = K3[dx + 1] * K3[dy + 1]
            gs = np.where(ok, gs + kk, gs)
            gv = np.where(ok, gv + kk * shift(var, step * dx, step * dy, f32(0)), gv)
    gv = gv / gs
    rl = f32(1) / (f32(p["sigma_luminance"]) * np.sqrt(gv) + f32(1e-4))
    lp = lum(e)
    sw = np.zeros_like(gz); sv = np.zeros_like(gz); se = np.zeros_like(e)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ok, num, den = pair(p, nz, m, gz, step, dx, dy)
            eq = shift(e, step * dx, step * dy, f32(0))
            vq = shift(var, step * dx, step * dy, f32(0))
            xl = np.abs(lp - lum(eq)) * rl
            w = ((H5[dx + 2] * H5[dy + 2]) * num) / (den * q(xl))
            sw = np.where(ok, sw + w, sw)
            se = np.where(ok[..., None], se + w[..., None] * eq, se)
            sv = np.where(ok, sv + (w * w) * vq, sv)
    return (se / sw[..., None]).astype(np.float32), (sv / (sw * sw)).astype(np.float32)


def denoise(acc, settings13, divide_by, normal, albedo, depth, material, hist=None, **params):
    """The restatement: acc int32[W, H, 3] (column-major, as dr_accum_read), guides as Context.render_aov returns them -> (f32[H, W, 3],
    uint8[H, W, 3]) in dr_accum_present's layout.  hist: the accumulator's history plane (int32[W, H]) -- pixel p then divides by
    hist[p] + divide_by, a divisor of 0 giving 0.  params: the fields of dr_denoise_params; any other name is a TypeError."""
    p = dict(DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError("unknown denoise parameter %r" % k)
        p[k] = v
    acc = np.asarray(acc, dtype=np.int32)
    W, H = acc.shape[0], acc.shape[1]
    gw, gh = grid(settings13, W, H)
    out = np.zeros((H, W, 3), np.float32)
    with np.errstate(all="ignore"):
        a = np.ascontiguousarray(acc[:gw, :gh].transpose(1, 0, 2)).astype(np.float32)
        if hist is None:
            c = a / f32(divide_by)
        else:
            n = (np.asarray(hist)[:gw, :gh].T.astype(np.int64) + int(divide_by)).astype(np.float32)[..., None]
            c = np.where(n == 0, f32(0), a / n).astype(np.float32)
        if p["iterations"] == 0:
            f = c
        else:
            m = np.asarray(material, np.int32)
            z = np.asarray(depth, np.float32)
            nz = np.concatenate([np.asarray(normal, np.float32), z[..., None]], axis=2)
            ap = albedo_prime(np.asarray(albedo, np.float32), m, p["demodulate"])
            gz = gradient(z, m)
            e = (c / ap).astype(np.float32)
            var = variance(p, nz, m, gz, lum(e))
            for i in range(p["iterations"]):
                e, var = atrous(p, nz, m, gz, e, var, 1 << i)
            f = (e * ap).astype(np.float32)
        out[:gh, :gw] = f
        rgb = np.fmin(np.fmax(out, f32(0)), f32(255)).astype(np.int32).astype(np.uint8)
    return out, rgb


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))
