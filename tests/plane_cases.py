"""Adversarial accumulator planes, seeded, shared by tests/test_planes_host.py (no GPU: proves that every case reaches the edge it is meant
for and that no reference compared by bits holds a NaN) and tests/test_gpu_planes.py (the same planes written into the live device planes with
tests/device_planes.py and run through the kernels).  Planes are indexed [x, y] like dr_accum_read: sums int32[W, H, 3], history int32[W, H],
second moments uint64[W, H].  Also the tables of cases both files walk, so that the CPU file checks exactly what the GPU file runs."""
import numpy as np

import moments_checks as mc
import reproject_checks as rc

INT_MAX = 2 ** 31 - 1
U64_MAX = 2 ** 64 - 1
STRIDE = 1000003

# accumulator W x H -> pixel grid: 141 x 99 -> 136 x 96 (smaller than the accumulator on both axes), 38 x 11 and 37 x 11 -> 32 x 8 (W * H % 4 = 2
# and 3: the scalar tail of the fused add; 141 x 99 has % 4 = 3 and 13 x 9 has 1), 13 x 9 -> 8 x 8, a single tile
BIG, TAIL2, TAIL3, TILE = (141, 99), (38, 11), (37, 11), (13, 9)
SIZES = (BIG, TAIL2, TAIL3, TILE)

# frames at the edge of the float -> int conversion of store_pixel: sky pixels above the luma cap, negative luma, beyond int32 either way,
# infinities (0 * inf = NaN -> 0 on black surfaces) and a NaN background
BACKGROUNDS = (3000.0, -3000.0, 1e7, -1e7, float("inf"), float("-inf"), float("nan"))
FRAME_SIZES = ((117, 89), TAIL3)
FRAME_SEEDS = (5, 1 + STRIDE * 3)

ADD_SEED = 31                                        # seeds ADD_SEED + STRIDE k: three frames at background 3000, then three at -3000
ADD_BACKGROUNDS = (3000.0, 3000.0, 3000.0, -3000.0, -3000.0, -3000.0)

ERROR_SIZES = (BIG, TAIL2, TILE)
ERROR_DIVIDE_BY = (0, 1, 2, 16)
ERROR_TOLERANCES = (0.0, 1.0, 1e9)

REPROJECT_SIZES = (BIG, TAIL2)
CARRIES = ((6, 4), (40, 8), (3, 5), (1, 65535), (9, 32))          # (frames, max_history)

DENOISE_SIZES = (BIG, TILE)
DENOISE_PARAMS = ({}, {"iterations": 10}, {"iterations": 1}, {"demodulate": 0}, {"normal_power_log2": 16}, {"sigma_luminance": 0.0}, {"material_stop": 0})
# acc_wide (|c| up to 2^31) goes through the parameter sets for which the host build was measured free of NaN and inf; acc_mixed through all
DENOISE_PARAMS_WIDE = ({}, {"iterations": 10}, {"demodulate": 0}, {"normal_power_log2": 16}, {"sigma_luminance": 0.0})
DENOISE_DIVIDE_BY = 3
PRESENT_DIVIDE_BY = (1, 3, 65535)                    # dr_accum_present refuses 0 (asserted); a history divisor of 0 is reached by dr_accum_error


def _rng(W, H, salt):
    return np.random.default_rng([W, H, salt])


def acc_wide(W, H, salt=0):
    """int32 uniform over the whole range"""
    return _rng(W, H, 100 + salt).integers(-2 ** 31, 2 ** 31, size=(W, H, 3), dtype=np.int64).astype(np.int32)


def acc_mixed(W, H, salt=0):
    """integers(-2^20, 2^20) times a per-pixel factor of 0, 1, 1, 256 or 2047: zeros, display-range sums, long-render sums and sums near the
    ends of int32, of both signs, side by side"""
    rng = _rng(W, H, 200 + salt)
    a = rng.integers(-2 ** 20, 2 ** 20, size=(W, H, 3), dtype=np.int64)
    return (a * rng.choice(np.array([0, 1, 1, 256, 2047], np.int64), size=(W, H, 1))).astype(np.int32)


def hist(W, H, salt=0):
    """integers(0, 70000), every fifth column 0: divisors of 0 (with divide_by 0), small ones and ones beyond 65535"""
    h = _rng(W, H, 300 + salt).integers(0, 70000, size=(W, H)).astype(np.int32)
    h[::5] = 0
    return h


def m2_wide(W, H, acc=None, salt=0):
    """uint64 uniform below 2^64; rows y = 1 mod 7 at or above 2^63, rows y = 3 mod 7 exactly 2^64 - 1, rows y = 5 mod 7 zero -- over non-zero
    sums where `acc` is given (a zero sum there is replaced by (1, -1, 1))"""
    m = _rng(W, H, 400 + salt).integers(0, 2 ** 64, size=(W, H), dtype=np.uint64)
    m[:, 1::7] |= np.uint64(2 ** 63)
    m[:, 3::7] = np.uint64(U64_MAX)
    m[:, 5::7] = 0
    if acc is not None:
        rows = acc[:, 5::7]
        rows[~rows.any(axis=2)] = (1, -1, 1)
    return m


def extreme(W, H):
    """the all-extreme planes of test_moments_host.py test_error_equals_the_restatement: sums of +-2^31 and 0, M2 of 2^64 - 1 and 0"""
    big_acc = np.full((W, H, 3), INT_MAX, np.int32)
    big_acc[::2] = -2 ** 31
    big_m2 = np.full((W, H), U64_MAX, np.uint64)
    big_m2[:, ::2] = 0
    big_acc[:, 1::4] = 0
    return big_acc, big_m2


def explicit_frame(W, H):
    """The explicit pixel list of test_moments_host.py test_add_cap_negative_values_and_saturation as (frame, m2 overrides {(x, y): value}):
    +-INT_MAX triples, y = 2^26 + 164 just capped and 2^26 - 19 just not, a negative pixel, and M2 values that stay at, pass and reach
    2^64 - 1 exactly.  A frame cannot be handed to the device's add (frames come from the render kernel), so the frame is for the host build;
    the GPU file installs the M2 values against the squares of the GPU's own first frame (saturating_m2)."""
    frame = _rng(W, H, 500).integers(-70000, 70000, size=(W, H, 3)).astype(np.int32)
    frame[0, 0] = (INT_MAX, INT_MAX, INT_MAX)
    frame[0, 1] = (-2 ** 31, -2 ** 31, -2 ** 31)
    frame[0, 2] = (0, 366716, 0)
    frame[0, 3] = (0, 366715, 0)
    frame[0, 4] = (-300, -5, -7)
    frame[1, 1] = (1, 1, 1)
    frame[1, 2] = (1, 1, 1)
    return frame, {(1, 0): U64_MAX, (1, 1): U64_MAX - 4, (1, 2): U64_MAX - 256 ** 2}


def saturating_m2(m2, first_square):
    """Installs the explicit list's three M2 values in place at the first three pixels (in memory order, rows that m2_wide does not stripe)
    where the first frame's square is not 0: 2^64 - 1 (stays), 2^64 - 5 (passes the end) and 2^64 - 1 - square (reaches 2^64 - 1 exactly,
    without wrapping).  Returns the three (x, y)."""
    W, H = m2.shape
    found = [(x, y) for x in range(W) for y in range(H) if y % 7 in (0, 2) and first_square[x, y] != 0][:3]
    assert len(found) == 3, "the first frame has fewer than three lit pixels"
    m2[found[0]] = np.uint64(U64_MAX)
    m2[found[1]] = np.uint64(U64_MAX - 4)
    m2[found[2]] = np.uint64(U64_MAX - int(first_square[found[2]]))
    return found


def fits_int32(acc, frames):
    """True when acc + frames[0] + ... stays inside int32 after every frame (the host build's += is signed)"""
    total = acc.astype(np.int64)
    for f in frames:
        total = total + f
        if total.max() > INT_MAX or total.min() < -2 ** 31:
            return False
    return True


def add_acc(W, H, frames):
    """acc_mixed with the first salt for which the sums of these frames stay inside int32 (asserted by the caller from its own reference)"""
    for salt in range(16):
        acc = acc_mixed(W, H, salt)
        if fits_int32(acc, frames):
            return acc
    raise AssertionError("no acc_mixed seed keeps the sums inside int32")


def trunc_div(a, d):
    """integer division towards zero, 0 where the divisor is 0"""
    a, d = a.astype(np.int64), np.broadcast_to(np.asarray(d).astype(np.int64), a.shape)
    safe = np.where(d == 0, 1, d)
    return np.where(d == 0, 0, np.sign(a) * np.sign(safe) * (np.abs(a) // np.abs(safe)))


def present(acc, history, div):
    """dr_accum_present restated (as tests/test_gpu_reproject.py _present): clamp(acc / (hist + div), 0, 255) towards zero, uint8[H, W, 3]"""
    return np.clip(trunc_div(acc, (history.astype(np.int64) + div)[..., None]), 0, 255).astype(np.uint8).transpose(1, 0, 2)


def error_cases(W, H):
    """(name, acc, hist or None, m2) of dr_accum_error's planes: acc_wide / acc_mixed x m2_wide x {no history, hist}, and the all-extreme pair"""
    out = []
    for name, make in (("wide", acc_wide), ("mixed", acc_mixed)):
        acc = make(W, H)
        m2 = m2_wide(W, H, acc)
        out.append((name, acc, None, m2))
        out.append((name + "+hist", acc, hist(W, H), m2))
    big_acc, big_m2 = extreme(W, H)
    out.append(("extreme", big_acc, None, big_m2))
    return out


def reproject_cases():
    """(frames, acc generator name, with the history plane, params) per move: the five carries over a history plane and the first two without
    one (as test_moments_host.py test_carry), sums alternating between acc_wide and acc_mixed, every second one with normal_cos 0.95, the
    last one with sky 0 (the masked class: the cube scene has one material, so only its sky can be masked)"""
    runs = [(f, mh, True) for f, mh in CARRIES] + [(f, mh, False) for f, mh in CARRIES[:2]]
    out = []
    for i, (f, mh, h) in enumerate(runs):
        params = {"max_history": mh}
        if i % 2:
            params["normal_cos"] = 0.95
        if i == len(runs) - 1:
            params["sky"] = 0
        out.append((f, "wide" if i % 2 == 0 else "mixed", h, params))
    return out


def denoise_cases():
    """(acc generator name, params) of the denoiser's runs"""
    return [("mixed", p) for p in DENOISE_PARAMS] + [("wide", p) for p in DENOISE_PARAMS_WIDE]


def make_acc(name, W, H):
    return {"wide": acc_wide, "mixed": acc_mixed}[name](W, H)


def add_inputs(W, H, frames):
    """(acc, m2, the three saturating pixels) the fused add starts from, given the six frames"""
    acc = add_acc(W, H, frames)
    m2 = m2_wide(W, H, acc)
    return acc, m2, saturating_m2(m2, mc.square(frames[0]))


def reproject_views(scene, st, W, H):
    """{move: (settings13, guides)} of the identity and the five moves"""
    views = {"identity": st}
    views.update(rc.moves(st))
    return {k: (v, scene.aov(v, W, H)) for k, v in views.items()}


def reproject_planes(W, H):
    return {"wide": acc_wide(W, H), "mixed": acc_mixed(W, H), "hist": hist(W, H), "m2": m2_wide(W, H)}


def check_carry(rng, acc, history, m2, frames, mh, got):
    """M2 and the sums of up to 200 random valid pixels of an IDENTITY reprojection of (acc, history or None, m2) in Python integers:
    M2 * mh // cnt and the sums towards zero beyond max_history, as they are up to it.  got: (acc, hist, counts, m2) of the reprojection.
    Returns how many of the pixels looked at had cnt > max_history and how many had not."""
    acc_to, hist_to, counts, m2_to = got
    xs, ys = np.nonzero(hist_to)
    beyond = within = 0
    for i in rng.choice(len(xs), min(200, len(xs)), replace=False):
        x, y = int(xs[i]), int(ys[i])
        c = (int(history[x, y]) if history is not None else 0) + frames
        m = int(m2[x, y])
        assert int(m2_to[x, y]) == (m if c <= mh else m * mh // c), (frames, mh, x, y)
        for k in range(3):
            v = int(acc[x, y, k])
            assert int(acc_to[x, y, k]) == (v if c <= mh else (abs(v) * mh // c) * (1 if v >= 0 else -1)), (frames, mh, x, y, k)
        beyond += c > mh
        within += c <= mh
    return beyond, within


def denoise_guides(scene, st, W, H):
    a = scene.aov(st, W, H)
    return a["normal"], a["albedo"], a["depth"], a["material"]
