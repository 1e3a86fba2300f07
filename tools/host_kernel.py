"""ctypes binding of tools/libhostkernel.so: the product's device functions (dogeray_amd/csrc/device_core.hpp) compiled for the host
(tools/host_kernel.cpp).  Test and bench infrastructure -- never part of the product library."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
from dogeray_amd import kat_marshal      # noqa: E402  (the known-answer hooks' table and marshaller; loads no library)
_SO = os.path.join(_HERE, "libhostkernel.so")
_CSRC = os.path.join(_ROOT, "dogeray_amd", "csrc")
_SOURCES = [os.path.join(_HERE, "host_kernel.cpp")] + [os.path.join(_CSRC, f) for f in ("rts_reader.cpp", "bvh_builder.cpp", "linearise.cpp", "wide_builder.cpp", "capi_host.cpp")]
_lib = None


def build(force=False):
    deps = _SOURCES + [os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith((".h", ".hpp"))] + [os.path.join(_HERE, "host_kernel", f) for f in ("host_stubs.hpp", "host_prims.hpp")]
    if not force and os.path.exists(_SO) and all(os.path.getmtime(d) <= os.path.getmtime(_SO) for d in deps):
        return _SO
    cxx = "/opt/rocm/lib/llvm/bin/clang++"          # ext_vector_type (u32x4) is a clang extension
    if not os.path.exists(cxx):
        cxx = "clang++"
    # -ffp-contract=off as on the device; -mfma so that the explicit fmaf of the folded node test is one instruction
    cmd = [cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-pthread", "-DDR_HOST_BUILD=1",
           "-I" + os.path.join(_HERE, "host_kernel"), "-o", _SO] + _SOURCES
    subprocess.check_call(cmd)
    return _SO


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.hk_last_error.restype = C.c_char_p
        L.hk_scene_load.restype = C.c_void_p
        L.hk_scene_load.argtypes = [C.c_char_p, C.c_char_p]
        L.hk_scene_free.argtypes = [C.c_void_p]
        L.hk_has_wide.argtypes = [C.c_void_p]
        L.hk_wide_depth.argtypes = [C.c_void_p]
        L.hk_hit.restype = C.c_int
        L.hk_hit.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong] + [C.c_void_p] * 5
        L.hk_trace.restype = C.c_int
        L.hk_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_longlong] + [C.c_void_p] * 8
        L.hk_ray_surface.restype = C.c_int
        L.hk_ray_surface.argtypes = [C.c_void_p, C.c_int, C.c_longlong] + [C.c_void_p] * 9
        L.hk_trace_plan.restype = None
        L.hk_trace_plan.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.hk_trace_persistent_min_rays.restype = C.c_longlong
        L.hk_radiance.restype = C.c_int
        L.hk_radiance.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong] + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_float, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]
        L.hk_nearest.restype = C.c_int
        L.hk_nearest.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong] + [C.c_void_p] * 9 + [C.c_int]
        L.hk_nearest_brute.restype = C.c_int
        L.hk_nearest_brute.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 8 + [C.c_int]
        L.hk_nearest_prim.restype = None
        L.hk_nearest_prim.argtypes = [C.c_longlong] + [C.c_void_p] * 8
        L.hk_nearest_prims.restype = C.c_longlong
        L.hk_nearest_prims.argtypes = [C.c_void_p] * 8
        L.hk_nearest_records.restype = C.c_longlong
        L.hk_nearest_records.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.hk_allhits.restype = C.c_int
        L.hk_allhits.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_longlong] + [C.c_void_p] * 3 + [C.c_int] * 3 + [C.c_void_p] * 9 + [C.c_int]
        L.hk_allhits_brute.restype = C.c_int
        L.hk_allhits_brute.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 3 + [C.c_int] * 2 + [C.c_void_p] * 3 + [C.c_int]
        L.hk_allhits_plan.restype = None
        L.hk_allhits_plan.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.hk_allhits_persistent_min_rays.restype = C.c_longlong
        L.hk_radiance_plan.restype = None
        L.hk_radiance_plan.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.hk_radiance_persistent_min_rays.restype = C.c_longlong
        L.hk_wide_info.restype = C.c_int
        L.hk_wide_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.hk_check_uniform.restype = C.c_longlong
        L.hk_check_uniform.argtypes = [C.c_longlong, C.c_ulonglong]
        L.hk_ray_margin.restype = None
        L.hk_ray_margin.argtypes = [C.c_longlong, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p]
        L.hk_ray_margin_k.restype = None
        L.hk_ray_margin_k.argtypes = [C.c_longlong, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
        L.hk_cert_factor_k.restype = C.c_float
        L.hk_cert_factor_k.argtypes = [C.c_double]
        L.hk_wide_mu.restype = C.c_int
        L.hk_wide_mu.argtypes = [C.c_void_p, C.c_void_p]
        L.hk_cert_check.restype = C.c_int
        L.hk_cert_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_float, C.c_longlong, C.c_uint64, C.c_void_p, C.c_void_p]
        L.hk_tri_hit.restype = None
        L.hk_tri_hit.argtypes = [C.c_longlong] + [C.c_void_p] * 6
        L.hk_tri_hit_uv.restype = None
        L.hk_tri_hit_uv.argtypes = [C.c_longlong] + [C.c_void_p] * 7
        L.hk_tri_barycentrics.restype = None
        L.hk_tri_barycentrics.argtypes = [C.c_longlong] + [C.c_void_p] * 6
        L.hk_hit_inputs.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 8
        L.hk_check_reject.restype = C.c_longlong
        L.hk_check_reject.argtypes = [C.c_longlong, C.c_ulonglong, C.POINTER(C.c_double)]
        L.hk_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.hk_camera_entry.restype = C.c_int
        L.hk_camera_entry.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.hk_camera_entry_check.restype = C.c_int
        L.hk_camera_entry_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.hk_slab.restype = None
        L.hk_slab.argtypes = [C.c_longlong] + [C.c_void_p] * 5
        L.hk_wide_leaves.restype = C.c_longlong
        L.hk_wide_leaves.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong]
        L.hk_cert_levels.restype = C.c_int
        L.hk_cert_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_longlong, C.c_uint64, C.c_void_p, C.c_void_p]
        L.hk_aov.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 8 + [C.c_void_p] * 9
        L.hk_denoise.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_void_p]
        L.hk_camera_block.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hk_reproject.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 12 + [C.c_int]
        L.hk_denoise_m2.argtypes = L.hk_denoise.argtypes + [C.c_void_p]
        L.hk_upscale.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 14 + [C.c_int, C.c_void_p, C.c_void_p]
        L.hk_reproject_m2.argtypes = L.hk_reproject.argtypes + [C.c_void_p, C.c_void_p]
        L.hk_moments_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong]
        L.hk_error.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.hk_persistent_plan.restype = None
        L.hk_persistent_plan.argtypes = [C.POINTER(C.c_int), C.c_longlong, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.hk_persistent_can_store_per_frame.argtypes = [C.POINTER(C.c_int)]
        L.hk_persistent_builds.argtypes = [C.c_void_p, C.c_int]
        L.hk_plan_regions.argtypes = [C.c_int] * 6
        L.hk_plan_split_limit.argtypes = [C.c_int] * 4
        L.hk_plan_sky_split.argtypes = [C.POINTER(C.c_int), C.c_longlong, C.c_int, C.c_int, C.c_int]
        L.hk_sky_split.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hk_sky_pixel.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.hk_sky_units.restype = C.c_uint
        L.hk_sky_units.argtypes = [C.c_uint, C.c_int, C.c_int]
        L.hk_sky_unit.restype = None
        L.hk_sky_unit.argtypes = [C.c_uint, C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.hk_sky_units_render.restype = C.c_longlong
        L.hk_sky_units_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
        L.hk_kat_sample.argtypes = [C.c_longlong] + [C.c_void_p] * 7
        L.hk_kat_outside.argtypes = [C.c_longlong, C.c_void_p, C.c_void_p]
        L.hk_kat_tex.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 4
        L.hk_kat_bounce.argtypes = [C.c_void_p, C.c_longlong] + [C.c_void_p] * 12
        L.hk_kat_miss.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
        L.hk_kat_camera.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_longlong] + [C.c_void_p] * 6
        L.hk_kat_store.argtypes = [C.c_longlong, C.c_void_p, C.c_int, C.c_void_p]
        _lib = L
    return _lib


def _ok(rc):
    if rc != 0:
        raise RuntimeError(lib().hk_last_error().decode())


# dr_kat_sample, dr_kat_outside, dr_kat_camera, dr_kat_store on the host (hk_kat_*): the arguments, checks and results of dogeray_amd.Context.kat_*, by
# the same table and marshaller (dogeray_amd.KAT_HOOKS, kat_marshal) -- where a hook returns both forms the arrays have a leading axis of 2, [0] the
# plain functions, [1] what the persistent kernel runs.  The hooks that read a scene (kat_tex, kat_bounce, kat_miss) are methods of Scene.
def _kat(hook, arrays, head=(), mid=(), outs=lambda out: [a.ctypes.data for a in out]):
    """kat_marshal calling hk_kat_<hook>(*head, n, inputs, *mid, outs(output arrays))"""
    def call(n, ins, out):
        _ok(getattr(lib(), "hk_kat_" + hook)(*head, n, *ins, *mid, *outs(out)))
    return kat_marshal(hook, arrays, call)


def kat_sample(seed, warm, kind):
    return _kat("sample", (seed, warm, kind), outs=lambda out: [out[0][0].ctypes.data, out[1][0].ctypes.data, out[0][1].ctypes.data, out[1][1].ctypes.data])


def kat_outside(d2):
    return _kat("outside", (d2,))[0]


def kat_camera(settings13, W, H, frame_seed, stride, x, y, sample):
    st = np.array(settings13, dtype=np.float32, order="C")
    return _kat("camera", (x, y, sample), head=(st.ctypes.data, int(W), int(H), int(frame_seed) & (2 ** 64 - 1), int(stride) & 0xFFFFFFFF))


def kat_store(color, spp):
    return _kat("store", (color,), mid=(int(spp),))[0]


def slab(o, d, mn, mx):
    """device_intersect.hpp slab() on n ray / box pairs (hk_slab): int32[n], 1 where the ray enters the box"""
    o, d, mn, mx = (np.ascontiguousarray(a, dtype=np.float32) for a in (o, d, mn, mx))
    hit = np.zeros(o.shape[0], np.int32)
    lib().hk_slab(o.shape[0], o.ctypes.data, d.ctypes.data, mn.ctypes.data, mx.ctypes.data, hit.ctypes.data)
    return hit


def tri_hit_uv(o, d, v0, e1, e2):
    """device_intersect.hpp tri_hit in both forms on n ray / triangle pairs -> (t of the plain form, t and uv float32[n, 2] of the form that hands out
    the barycentrics)"""
    o, d, v0, e1, e2 = (np.ascontiguousarray(a, dtype=np.float32) for a in (o, d, v0, e1, e2))
    n = o.shape[0]
    t0, t1, uv = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 2), np.float32)
    lib().hk_tri_hit(n, o.ctypes.data, d.ctypes.data, v0.ctypes.data, e1.ctypes.data, e2.ctypes.data, t0.ctypes.data)
    lib().hk_tri_hit_uv(n, o.ctypes.data, d.ctypes.data, v0.ctypes.data, e1.ctypes.data, e2.ctypes.data, t1.ctypes.data, uv.ctypes.data)
    return t0, t1, uv


def tri_barycentrics(o, d, v0, e1, e2):
    """device_surface.hpp tri_barycentrics on n ray / triangle pairs -> float32[n, 2]: ux, uy as surface_normal forms them"""
    o, d, v0, e1, e2 = (np.ascontiguousarray(a, dtype=np.float32) for a in (o, d, v0, e1, e2))
    uv = np.zeros((o.shape[0], 2), np.float32)
    lib().hk_tri_barycentrics(o.shape[0], o.ctypes.data, d.ctypes.data, v0.ctypes.data, e1.ctypes.data, e2.ctypes.data, uv.ctypes.data)
    return uv


def hit_inputs(o, d, t, uv, prims, shade, seed, form=0, carried=False, lazy=False, tex=None, texels=None):
    """hk_hit_inputs: what the shade phase forms at n hits.  prims uint32[n, 12] (DevPrim words), shade uint32[n, 32] (DevShade words), tex int32[k, 4]
    (DevTex words) with texels uint32[...]; form 0 = shade_prepare, form 1 = shade_prepare_hit<carried, lazy> -> dict of alive int32[n],
    texco float32[n, 2], sc uint32[n, 16] (the words of ShadeCtx), emitted float32[n, 3], next uint32[n, 2]."""
    o, d, t, uv = (np.ascontiguousarray(a, dtype=np.float32) for a in (o, d, t, uv))
    prims, shade = np.ascontiguousarray(prims, dtype=np.uint32), np.ascontiguousarray(shade, dtype=np.uint32)
    seed = np.ascontiguousarray(seed, dtype=np.uint64)
    n = o.shape[0]
    assert prims.shape == (n, 12) and shade.shape == (n, 32) and uv.shape == (n, 2) and t.shape == (n,) and seed.shape == (n,)
    tex = np.ascontiguousarray(tex if tex is not None else np.zeros((1, 4)), dtype=np.int32)
    texels = np.ascontiguousarray(texels if texels is not None else np.zeros(1), dtype=np.uint32)
    out = {"alive": np.zeros(n, np.int32), "texco": np.zeros((n, 2), np.float32), "sc": np.zeros((n, 16), np.uint32), "emitted": np.zeros((n, 3), np.float32),
           "next": np.zeros((n, 2), np.uint32)}
    _ok(lib().hk_hit_inputs(n, int(form), int(bool(carried)), int(bool(lazy)), o.ctypes.data, d.ctypes.data, t.ctypes.data, uv.ctypes.data, prims.ctypes.data,
                            shade.ctypes.data, int(tex.shape[0]) if texels.size > 1 else 0, tex.ctypes.data, texels.ctypes.data, seed.ctypes.data,
                            out["alive"].ctypes.data, out["texco"].ctypes.data, out["sc"].ctypes.data, out["emitted"].ctypes.data, out["next"].ctypes.data))
    return out


NEAREST_CHANNELS = ("distance", "d2", "object", "material", "point", "uv")      # in the order of dr_nearest_buffers


def _nearest_in(p, rmax):
    p = np.ascontiguousarray(p, dtype=np.float32)
    n = p.shape[0]
    assert p.shape == (n, 3)
    if rmax is not None:
        rmax = np.ascontiguousarray(rmax, dtype=np.float32)
        assert rmax.shape == (n,)
    return p, rmax, n


def _nearest_out(n, channels):
    shape = {"distance": (n,), "d2": (n,), "object": (n,), "material": (n,), "point": (n, 3), "uv": (n, 2)}
    return {k: np.zeros(shape[k], np.int32 if k in ("object", "material") else np.float32) for k in channels}


ALLHITS_CHANNELS = ("count", "t", "object", "material", "distance", "normal", "uv", "albedo")      # in the order of dr_allhits_buffers
_ALLHITS_SPEC = {"count": (np.int32, 0), "t": (np.float32, 1), "object": (np.int32, 1), "material": (np.int32, 1), "distance": (np.float32, 1),
                 "normal": (np.float32, 3), "uv": (np.float32, 2), "albedo": (np.float32, 3)}


def _allhits_in(o, d, tmax):
    o, d = np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)
    n = o.shape[0]
    assert o.shape == (n, 3) and d.shape == (n, 3)
    if tmax is not None:
        tmax = np.ascontiguousarray(tmax, dtype=np.float32)
        assert tmax.shape == (n,)
    return o, d, tmax, n


def _allhits_out(n, K, channels):
    K = max(K, 0)      # (a K out of range is refused by the library)
    shape = lambda c: (n,) if c == 0 else ((n, K) if c == 1 else (n, K, c))
    return {k: np.zeros(shape(_ALLHITS_SPEC[k][1]), _ALLHITS_SPEC[k][0]) for k in channels}


def allhits_max():
    """DR_ALLHITS_MAX as the device code sees it"""
    return int(lib().hk_allhits_max())


def allhits_chunk():
    """rays a wave of the persistent kernel takes from the list per atomic (launch_plan.hpp ALLHITS_CHUNK)"""
    return int(lib().hk_allhits_chunk())


def allhits_plan(n, has_wide, num_cus=256, force=0):
    """launch_plan.hpp plan_allhits -> (kernel: 0 one ray per lane / 1 persistent, wide 1 / 0, workgroups)"""
    out = (C.c_int * 3)()
    lib().hk_allhits_plan(int(n), int(bool(has_wide)), int(num_cus), int(force), out)
    return tuple(out)


def allhits_persistent_min_rays():
    return int(lib().hk_allhits_persistent_min_rays())


def nearest_k():
    """the k of the accuracy bound k u (d + 2 Lmax) of nearest_prim (device_nearest.hpp NEAREST_K)"""
    return int(lib().hk_nearest_k())


def nearest_prim(kind, a, b, c, p):
    """nearest_prim (device_nearest.hpp) pair by pair -> (d2 [n], q [n, 3], uv [n, 2])"""
    kind = np.ascontiguousarray(kind, np.int32)
    a, b, c, p = (np.ascontiguousarray(x, np.float32) for x in (a, b, c, p))
    n = len(kind)
    d2, q, uv = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 2), np.float32)
    lib().hk_nearest_prim(n, kind.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data, p.ctypes.data, d2.ctypes.data, q.ctypes.data, uv.ctypes.data)
    return d2, q, uv


class Scene:
    def __init__(self, rts_path, texdir=""):
        self.h = lib().hk_scene_load(os.fsencode(rts_path), os.fsencode(texdir or ""))
        if not self.h:
            raise RuntimeError(lib().hk_last_error().decode())

    def __del__(self):
        try:
            if self.h:
                lib().hk_scene_free(self.h)
                self.h = None
        except Exception:
            pass

    @property
    def has_wide(self):
        return bool(lib().hk_has_wide(self.h))

    def wide_depth(self):
        return int(lib().hk_wide_depth(self.h))

    def hit(self, o, d, traversal=2, tree=2, want_visits=False):
        """dr_kat_hit on the host (hk_hit): the closest hits of the rays (o, d) by the walk of `traversal` (0 threaded, 1 ordered, 2 wide) over the tree
        of wide_tree = `tree` (1 / 2) -> (t float32[n], -1 on a miss; original object index int32[n], 0 on a miss[; boxes tested int32[n]])."""
        o, d = np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)
        n = o.shape[0]
        assert o.shape == (n, 3) and d.shape == (n, 3)
        t, idx = np.zeros(n, np.float32), np.zeros(n, np.int32)
        vis = np.zeros(n, np.int32) if want_visits else None
        if lib().hk_hit(self.h, int(traversal), int(tree), n, o.ctypes.data, d.ctypes.data, t.ctypes.data, idx.ctypes.data,
                        vis.ctypes.data if want_visits else None) != 0:
            raise RuntimeError(lib().hk_last_error().decode())
        return (t, idx, vis) if want_visits else (t, idx)

    def trace(self, o, d, tmax=None, traversal=2, tree=2, any_hit=False, channels=("t", "object"), want_visits=False):
        """dr_trace_rays on the host (hk_trace, hk_ray_surface): the rays (o, d[, tmax]) by the walks of device_trace.hpp -> a dict of arrays as
        dogeray_amd.Context.trace returns it ({"occluded"} for any_hit); want_visits adds "visits", the boxes tested per ray."""
        o, d = np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)
        n = o.shape[0]
        assert o.shape == (n, 3) and d.shape == (n, 3)
        if tmax is not None:
            tmax = np.ascontiguousarray(tmax, dtype=np.float32)
            assert tmax.shape == (n,)
        t, idx, slot, occ = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        vis = np.zeros(n, np.int32)
        if lib().hk_trace(self.h, int(traversal), int(tree), 1 if any_hit else 0, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data if tmax is not None else None,
                          t.ctypes.data, idx.ctypes.data, occ.ctypes.data, slot.ctypes.data, vis.ctypes.data) != 0:
            raise RuntimeError(lib().hk_last_error().decode())
        if any_hit:
            out = {"occluded": occ}
        else:
            out = {}
            sizes = {"material": (np.int32, 1), "distance": (np.float32, 1), "normal": (np.float32, 3), "uv": (np.float32, 2), "albedo": (np.float32, 3)}
            extra = {k: np.zeros((n, sizes[k][1]) if sizes[k][1] > 1 else n, sizes[k][0]) for k in channels if k in sizes}
            if extra:
                if lib().hk_ray_surface(self.h, int(tree), n, o.ctypes.data, d.ctypes.data, t.ctypes.data, slot.ctypes.data,
                                        *[extra[k].ctypes.data if k in extra else None for k in ("material", "distance", "normal", "uv", "albedo")]) != 0:
                    raise RuntimeError(lib().hk_last_error().decode())
            for k in channels:
                out[k] = t if k == "t" else idx if k == "object" else extra[k]
        if want_visits:
            out["visits"] = vis
        return out

    def radiance(self, o, d, spp=1, max_depth=10, background=1.0, backtex=-1, seed=0, seeds=None, skip=None, traversal=2, tree=2,
                 channels=("radiance", "bounces")):
        """dr_trace_radiance on the host (hk_radiance: device_radiance.hpp radiance_ray over the host walks): the arguments and the dict of
        dogeray_amd.Context.radiance, by the walk of `traversal` over the tree of wide_tree = `tree`."""
        o, d = np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)
        n = o.shape[0]
        assert o.shape == (n, 3) and d.shape == (n, 3)
        seeds = None if seeds is None else np.ascontiguousarray(seeds, np.uint64)
        skip = None if skip is None else np.ascontiguousarray(skip, np.int32)
        assert (seeds is None or seeds.shape == (n,)) and (skip is None or skip.shape == (n,))
        out = {k: np.zeros((n, 3), np.float32) if k == "radiance" else np.zeros(n, np.int32) for k in channels}
        _ok(lib().hk_radiance(self.h, int(traversal), int(tree), n, o.ctypes.data, d.ctypes.data, seeds.ctypes.data if seeds is not None else None,
                              skip.ctypes.data if skip is not None else None, int(spp), int(max_depth), float(background), int(backtex),
                              int(seed) & (2 ** 64 - 1), out["radiance"].ctypes.data if "radiance" in out else None,
                              out["bounces"].ctypes.data if "bounces" in out else None))
        return out

    def nearest(self, p, rmax=None, walk=2, tree=2, channels=NEAREST_CHANNELS, want_visits=False, nthreads=1):
        """dr_query_nearest on the host (hk_nearest): the points p[, rmax] by the walks of device_nearest.hpp -- walk 2 the 4-way records of the tree of
        wide_tree = `tree`, 0 the threaded links -> a dict of arrays as dogeray_amd.Context.nearest returns it; want_visits adds "visits", the records
        visited per query."""
        p, rmax, n = _nearest_in(p, rmax)
        out = _nearest_out(n, channels)
        vis = np.zeros(n, np.int32)
        _ok(lib().hk_nearest(self.h, int(walk), int(tree), n, p.ctypes.data, rmax.ctypes.data if rmax is not None else None,
                             *[out[k].ctypes.data if k in out else None for k in NEAREST_CHANNELS], vis.ctypes.data, int(nthreads)))
        if want_visits:
            out["visits"] = vis
        return out

    def nearest_brute(self, p, rmax=None, channels=NEAREST_CHANNELS, nthreads=1):
        """the same answer by its definition (hk_nearest_brute): the key-minimum of nearest_prim over every primitive, no tree"""
        p, rmax, n = _nearest_in(p, rmax)
        out = _nearest_out(n, channels)
        _ok(lib().hk_nearest_brute(self.h, n, p.ctypes.data, rmax.ctypes.data if rmax is not None else None,
                                   *[out[k].ctypes.data if k in out else None for k in NEAREST_CHANNELS], int(nthreads)))
        return out

    def nearest_prims(self):
        """the primitive records in slot order: dict kind (0 sphere, 1 triangle, 2 none), a, b, c [n, 3], orig, material, and lmax (the pruning slack's scene constant)"""
        n = int(lib().hk_nearest_prims(self.h, *([None] * 7)))
        kind, orig, mat = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        a, b, c = (np.zeros((n, 3), np.float32) for _ in range(3))
        lmax = np.zeros(1, np.float32)
        lib().hk_nearest_prims(self.h, kind.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data, orig.ctypes.data, mat.ctypes.data, lmax.ctypes.data)
        return {"kind": kind, "a": a, "b": b, "c": c, "orig": orig, "material": mat, "lmax": float(lmax[0])}

    def nearest_records(self, walk=2, tree=2):
        """records of the walk Scene.nearest takes"""
        return int(lib().hk_nearest_records(self.h, int(walk), int(tree)))

    def allhits(self, o, d, tmax=None, max_hits=4, kind_mask=3, walk=2, tree=2, channels=("count", "t", "object"), zero_margin=False, want_visits=False,
                nthreads=1):
        """dr_trace_all_hits on the host (hk_allhits): the rays (o, d[, tmax]) by the walks of device_allhits.hpp -- walk 2 the 4-way records of the tree
        of wide_tree = `tree`, 0 the threaded links -> a dict of arrays as dogeray_amd.Context.trace_all returns it; zero_margin forces the wide node
        step's margins to zero (the switch of tests/test_allhits_host.py); want_visits adds "visits", the records visited per ray."""
        o, d, tmax, n = _allhits_in(o, d, tmax)
        out = _allhits_out(n, int(max_hits), channels)
        vis = np.zeros(n, np.int32)
        _ok(lib().hk_allhits(self.h, int(walk), int(tree), n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data if tmax is not None else None, int(max_hits),
                             int(kind_mask), int(bool(zero_margin)), *[out[k].ctypes.data if k in out else None for k in ALLHITS_CHANNELS], vis.ctypes.data,
                             int(nthreads)))
        if want_visits:
            out["visits"] = vis
        return out

    def allhits_brute(self, o, d, tmax=None, max_hits=4, kind_mask=3, nthreads=1):
        """the same answer by its definition (hk_allhits_brute): a loop over every leaf record, no walk -> {"count", "t", "object"}"""
        o, d, tmax, n = _allhits_in(o, d, tmax)
        out = _allhits_out(n, int(max_hits), ("count", "t", "object"))
        _ok(lib().hk_allhits_brute(self.h, n, o.ctypes.data, d.ctypes.data, tmax.ctypes.data if tmax is not None else None, int(max_hits), int(kind_mask),
                                   out["count"].ctypes.data, out["t"].ctypes.data, out["object"].ctypes.data, int(nthreads)))
        return out

    def kat_tex(self, tex, u, v):
        return _kat("tex", (tex, u, v), head=(self.h,))[0]

    def kat_bounce(self, obj_index, o, d, t, atten, seed, warm):
        return _kat("bounce", (obj_index, o, d, t, atten, seed, warm), head=(self.h,))

    def kat_miss(self, d, atten, backtex, background):
        return _kat("miss", (d, atten), head=(self.h,), mid=(int(backtex), float(background)))[0]

    def wide_info(self, tree=2):
        """What dr_context_get_option reports for the tree of wide_tree = `tree`: a dict with wide_depth (0: no wide tree), wide_own_bounds, wide_nodes."""
        out = np.zeros(3, np.int32)
        if lib().hk_wide_info(self.h, int(tree), out.ctypes.data) != 0:
            raise RuntimeError(lib().hk_last_error().decode())
        return {"wide_depth": int(out[0]), "wide_own_bounds": int(out[1]), "wide_nodes": int(out[2])}

    def render(self, settings13, W, H, background, frame_seed, traversal=2, nthreads=1, col_mod=1, col_rem=0, count=True, level_plane=None, cert_factor=40,
               graded=1, entry_plane=None):
        """One frame: (int32[W, H, 3] indexed [x, y], counters dict or None).  level_plane: the grades of the view's grazing certificate
        (cert_levels()[0] for the same cert_factor / graded) -- the frame is rendered over the default tree with the camera rays' certified margins.
        entry_plane: the entry codes of the view's camera rays (camera_entry()[0] for the same stripe): they start their walks there."""
        st = np.ascontiguousarray(settings13, dtype=np.float32)
        out = np.zeros((W, H, 3), dtype=np.int32)
        ctr = (C.c_uint64 * 6)()
        plane = np.ascontiguousarray(level_plane, dtype=np.uint8) if level_plane is not None else None
        eplane = np.ascontiguousarray(entry_plane, dtype=np.int32) if entry_plane is not None else None
        rc = lib().hk_render(self.h, st.ctypes.data, W, H, float(background), int(frame_seed) & (2 ** 64 - 1), traversal, nthreads, col_mod, col_rem,
                             out.ctypes.data, C.cast(ctr, C.c_void_p) if count else None,
                             plane.ctypes.data if plane is not None else None, int(cert_factor), int(graded),
                             eplane.ctypes.data if eplane is not None else None)
        if rc != 0:
            raise RuntimeError(lib().hk_last_error().decode())
        return out, (dict(zip(("rays", "V", "L", "S", "T", "samples"), [int(v) for v in ctr])) if count else None)

    def camera_entry(self, settings13, W, H, col_mod=1, col_rem=0, mutant=0):
        """The camera rays' entry table of a view on the host (hk_camera_entry): (int32 entry codes, a word per tile of the stripe, and a dict of counts),
        or None when the view or the scene gives no table.  mutant: one of device_cert.hpp's wrong rules (1 rect narrowed, 2 no lens term, 3 highest
        rank off by one, 4 no entry for a tile with one leaf)."""
        st = np.ascontiguousarray(settings13, dtype=np.float32)
        div = int(st[11]) if np.isfinite(st[11]) and st[11] >= 1 else 1
        gx, gy = W // div // 8, H // div // 8
        ncols = (gx - col_rem + col_mod - 1) // col_mod if gx > col_rem else 0
        codes = np.zeros(max(1, ncols * gy), np.int32)
        out = np.zeros(32, np.int64)
        rc = lib().hk_camera_entry(self.h, st.ctypes.data, W, H, int(col_mod), int(col_rem), int(mutant), codes.ctypes.data, out.ctypes.data)
        if rc < 0:
            raise RuntimeError(lib().hk_last_error().decode())
        if rc != 0:
            return None
        assert int(out[0]) == ncols * gy
        return codes[:ncols * gy], {"tiles": int(out[0]), "none": int(out[1]), "root": int(out[2]), "leaf": int(out[3]), "every": int(out[4]), "leaves": int(out[5]),
                                    "depth": [int(v) for v in out[8:26]]}

    def camera_entry_check(self, settings13, W, H, codes, seed, stride, frames, col_mod=1, col_rem=0, nthreads=8):
        """hk_camera_entry_check: the kernel's camera rays of `frames` frames against every leaf, by brute force -> dict rays, entered, outside (leaves
        entered that do not lie under their tile's entry: must be 0), entered_below_root."""
        st = np.ascontiguousarray(settings13, dtype=np.float32)
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        out = np.zeros(4, np.int64)
        if lib().hk_camera_entry_check(self.h, st.ctypes.data, W, H, int(col_mod), int(col_rem), int(seed), int(stride), int(frames), int(nthreads),
                                       codes.ctypes.data, out.ctypes.data) != 0:
            raise RuntimeError(lib().hk_last_error().decode())
        return {"rays": int(out[0]), "entered": int(out[1]), "outside": int(out[2]), "entered_below_root": int(out[3])}

    def sky_pixel(self, settings13, W, H, background, seed, stride, frames, xs, ys):
        """device_sky.hpp sky_pixel for the pixels (xs, ys), summed over `frames` frames of a launch with dr_render_accumulate's seed and stride
        (hk_sky_pixel): int32[n, 3], what those frames add to the accumulator when every path of the pixels misses."""
        st = np.ascontiguousarray(settings13, dtype=np.float32)
        xs, ys = np.ascontiguousarray(xs, dtype=np.int32), np.ascontiguousarray(ys, dtype=np.int32)
        out = np.zeros((len(xs), 3), np.int32)
        if lib().hk_sky_pixel(self.h, st.ctypes.data, W, H, float(background), int(seed) & (2 ** 64 - 1), int(stride) & (2 ** 64 - 1), int(frames), len(xs),
                              xs.ctypes.data, ys.ctypes.data, out.ctypes.data) != 0:
            raise RuntimeError(lib().hk_last_error().decode())
        return out

    def sky_units_render(self, settings13, W, H, background, seed, stride, batch, chunk, sky_list, perm=None, cost=None):
        """device_sky.hpp sky_tile_frames over every unit of a launch of `batch` frames whose sky tiles are sky_list (hk_sky_units_render), the units in
        the order perm gives: (int32[W, H, 3] what the units add to an accumulator of zeros, units run).  cost: uint32[tiles * 64], written in place."""
        st = np.ascontiguousarray(settings13, dtype=np.float32)
        sl = np.ascontiguousarray(sky_list, dtype=np.int32)
        pm = np.ascontiguousarray(perm, dtype=np.uint32) if perm is not None else None
        acc = np.zeros((W, H, 3), np.int32)
        n = lib().hk_sky_units_render(self.h, st.ctypes.data, W, H, float(background), int(seed) & (2 ** 64 - 1), int(stride) & (2 ** 64 - 1), int(batch),
                                      int(chunk), len(sl), sl.ctypes.data, pm.ctypes.data if pm is not None else None, acc.ctypes.data,
                                      cost.ctypes.data if cost is not None else None)
        if n < 0:
            raise RuntimeError(lib().hk_last_error().decode())
        return acc, int(n)

    def wide_leaves(self):
        """The default tree's leaves in depth-first order: (uint32 record per rank, float32 (n, 6) box per rank -- mn, mx of the record --, uint32 (records, 2)
        rank range per record)."""
        n = int(lib().hk_wide_leaves(self.h, None, None, None, 0, 0))
        if n < 0:
            raise RuntimeError(lib().hk_last_error().decode())
        nrec = self.wide_info(2)["wide_nodes"] + n
        rec, boxes, rng = np.zeros(n, np.uint32), np.zeros((n, 6), np.float32), np.zeros((nrec, 2), np.uint32)
        lib().hk_wide_leaves(self.h, rec.ctypes.data, boxes.ctypes.data, rng.ctypes.data, n, nrec)
        return rec, boxes, rng

    def wide_mu(self):
        """(own-bounds triangles, float32 (e, l, v)) of the product's default tree (hk_wide_mu)."""
        mu = np.zeros(3, np.float32)
        return int(lib().hk_wide_mu(self.h, mu.ctypes.data)), mu

    def cert_levels(self, settings13, W, H, cert_factor=40, graded=1, e_own=1e30, n_samples=0, seed=1):
        """The graded grazing certificate of a view on the host (hk_cert_levels): (uint8 grades, a byte per tile, and a dict of the sampling check's
        counts), or None when the view gives no certificate."""
        st = np.ascontiguousarray(settings13, dtype=np.float32)
        div = int(st[11]) if np.isfinite(st[11]) and st[11] >= 1 else 1
        plane = np.zeros((W // div // 8) * (H // div // 8), np.uint8)
        out = np.zeros(24, np.int64)
        if lib().hk_cert_levels(self.h, st.ctypes.data, W, H, int(cert_factor), int(graded), C.c_float(e_own), int(n_samples), int(seed), out.ctypes.data,
                                plane.ctypes.data) != 0:
            return None
        return plane, {"rays_certified": int(out[0]), "below_step": int(out[1]), "rays_constrained": int(out[2]), "tile_above": int(out[3]),
                       "n_levels": int(out[4]), "tiles": int(out[5]), "every": int(out[6]), "base": int(out[7]),
                       "tiles_per_grade": [int(v) for v in out[8:16]], "rays_per_grade": [int(v) for v in out[16:24]]}

    def aov(self, settings13, W, H, window=None, traversal=2, nthreads=4):
        """dr_render_aov on the host (device_aov.hpp aov_first_hit): every channel of the window (x0, y0, w, h) of the pixel grid
        (None: all of it) as a dict of arrays shaped like dogeray_amd.Context.render_aov's."""
        st = np.ascontiguousarray(settings13, dtype=np.float32)
        if window is None:
            div = int(st[11])
            window = (0, 0, W // div // 8 * 8, H // div // 8 * 8)
        x0, y0, w, h = (int(v) for v in window)
        out = {"t": np.zeros((h, w), np.float32), "distance": np.zeros((h, w), np.float32), "depth": np.zeros((h, w), np.float32),
               "object": np.zeros((h, w), np.int32), "material": np.zeros((h, w), np.int32), "normal": np.zeros((h, w, 3), np.float32),
               "uv": np.zeros((h, w, 2), np.float32), "albedo": np.zeros((h, w, 3), np.float32), "dir": np.zeros((h, w, 3), np.float32)}
        rc = lib().hk_aov(self.h, st.ctypes.data, W, H, x0, y0, w, h, traversal, nthreads,
                          *[out[k].ctypes.data for k in ("t", "distance", "depth", "object", "material", "normal", "uv", "albedo", "dir")])
        if rc != 0:
            raise RuntimeError(lib().hk_last_error().decode())
        return out


DENOISE_DEFAULTS = {"iterations": 5, "sigma_luminance": 4.0, "normal_power_log2": 7, "sigma_depth": 1.0, "demodulate": 1, "material_stop": 1}


def denoise(acc, settings13, divide_by, normal, albedo, depth, material, nthreads=4, hist=None, m2=None, **params):
    """dr_accum_denoise on the host (device_denoise.hpp): the accumulator acc (int32[W, H, 3], column-major as dr_accum_read returns it) and the
    guides as arrays shaped like dogeray_amd.Context.render_aov's (normal / albedo [gh, gw, 3], depth / material [gh, gw]) -> (f32[H, W, 3],
    uint8[H, W, 3]) in dr_accum_present's layout.  hist: the accumulator's history plane (int32[W, H], dr_accum_history_read) -- pixel p then
    divides by hist[p] + divide_by.  m2: the second-moment plane (uint64[W, H], dr_accum_moments_read) -- option "denoise_variance" = 1: pixels with
    four samples or more take their variance from it.  params: the fields of dr_denoise_params (the rest default)."""
    acc = np.ascontiguousarray(acc, dtype=np.int32)
    W, H = acc.shape[0], acc.shape[1]
    st = np.ascontiguousarray(settings13, dtype=np.float32)
    p = dict(DENOISE_DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError("unknown denoise parameter %r" % k)
        p[k] = v
    raw = np.array([p["iterations"], 0, p["normal_power_log2"], 0, p["demodulate"], p["material_stop"]], dtype=np.int32)
    raw[1] = np.array([p["sigma_luminance"]], np.float32).view(np.int32)[0]
    raw[3] = np.array([p["sigma_depth"]], np.float32).view(np.int32)[0]
    guides = [np.ascontiguousarray(a, dtype=t) for a, t in ((normal, np.float32), (albedo, np.float32), (depth, np.float32), (material, np.int32))]
    f32 = np.zeros((H, W, 3), np.float32)
    rgb = np.zeros((H, W, 3), np.uint8)
    if hist is not None:
        hist = np.ascontiguousarray(hist, dtype=np.int32)
        assert hist.shape == (W, H)
    if m2 is not None:
        m2 = np.ascontiguousarray(m2, dtype=np.uint64)
        assert m2.shape == (W, H)
    rc = lib().hk_denoise_m2(acc.ctypes.data, W, H, int(divide_by), st.ctypes.data, *[g.ctypes.data for g in guides], raw.ctypes.data,
                             f32.ctypes.data, rgb.ctypes.data, nthreads, hist.ctypes.data if hist is not None else None,
                             m2.ctypes.data if m2 is not None else None)
    if rc != 0:
        raise RuntimeError(lib().hk_last_error().decode())
    return f32, rgb


UPSCALE_DEFAULTS = {"mode": 1, "normal_power_log2": 5, "sigma_depth": 1.0, "demodulate": 1, "material_stop": 1}


def _denoise_raw(p):
    raw = np.array([p["iterations"], 0, p["normal_power_log2"], 0, p["demodulate"], p["material_stop"]], dtype=np.int32)
    raw[1] = np.array([p["sigma_luminance"]], np.float32).view(np.int32)[0]
    raw[3] = np.array([p["sigma_depth"]], np.float32).view(np.int32)[0]
    return raw


def upscale(acc, settings13, divide_by, low_guides, full_guides, hist=None, m2=None, prefilter=None, nthreads=4, **params):
    """dr_accum_upscale on the host (device_upscale.hpp): the accumulator acc (int32[W, H, 3] as dr_accum_read returns it), the guides of
    settings13 (low_guides) and of settings13 with element 11 = 1 (full_guides) as dicts with "normal", "albedo", "depth", "material" shaped like
    dogeray_amd.Context.render_aov's (block mode reads neither: both may be None) -> (f32[H, W, 3], uint8[H, W, 3], no-tap mask bool[H, W]) in
    dr_accum_present's layout.  hist / m2 as denoise(); prefilter: None, or a dict of dr_denoise_params fields (the rest default) -- the
    denoiser's host passes run on the low grid first; params: the fields of dr_upscale_params (the rest default)."""
    acc = np.ascontiguousarray(acc, dtype=np.int32)
    W, H = acc.shape[0], acc.shape[1]
    st = np.ascontiguousarray(settings13, dtype=np.float32)
    p = dict(UPSCALE_DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError("unknown upscale parameter %r" % k)
        p[k] = v
    raw = np.array([p["mode"], p["normal_power_log2"], 0, p["demodulate"], p["material_stop"]], dtype=np.int32)
    raw[2] = np.array([p["sigma_depth"]], np.float32).view(np.int32)[0]
    pre = None
    if prefilter is not None:
        d = dict(DENOISE_DEFAULTS)
        for k, v in dict(prefilter).items():
            if k not in d:
                raise TypeError("unknown denoise parameter %r" % k)
            d[k] = v
        pre = _denoise_raw(d)
    keep = []

    def ptrs(g, shape):
        if g is None:
            return [None] * 4
        out = []
        for k, t in (("normal", np.float32), ("albedo", np.float32), ("depth", np.float32), ("material", np.int32)):
            a = np.ascontiguousarray(g[k], dtype=t)
            assert a.shape[:2] == shape, "guides are not the %d x %d pixel grid" % (shape[1], shape[0])
            keep.append(a)
            out.append(a.ctypes.data)
        return out
    div = int(st[11]) if np.isfinite(st[11]) and st[11] >= 1 else 1
    low = ptrs(low_guides, (H // div // 8 * 8, W // div // 8 * 8))
    full = ptrs(full_guides, (H // 8 * 8, W // 8 * 8))
    f32 = np.zeros((H, W, 3), np.float32)
    rgb = np.zeros((H, W, 3), np.uint8)
    notap = np.zeros((H, W), np.uint8)
    if hist is not None:
        hist = np.ascontiguousarray(hist, dtype=np.int32)
        assert hist.shape == (W, H)
    if m2 is not None:
        m2 = np.ascontiguousarray(m2, dtype=np.uint64)
        assert m2.shape == (W, H)
    rc = lib().hk_upscale(acc.ctypes.data, W, H, int(divide_by), st.ctypes.data, *low, *full, raw.ctypes.data, pre.ctypes.data if pre is not None else None,
                          f32.ctypes.data, rgb.ctypes.data, notap.ctypes.data, nthreads, hist.ctypes.data if hist is not None else None,
                          m2.ctypes.data if m2 is not None else None)
    if rc != 0:
        raise RuntimeError(lib().hk_last_error().decode())
    return f32, rgb, notap.astype(bool)


def camera_block(settings13, W, H):
    """The float camera block of a view as the library forms it from settings13 (params_host.hpp fill_view_params): a dict with float32
    "from", "llc", "hor", "ver", float64 "den_w", "den_h" and the pixel grid "gw", "gh"."""
    st = np.ascontiguousarray(settings13, dtype=np.float32)
    out, den, grid = np.zeros(12, np.float32), np.zeros(2, np.float64), np.zeros(2, np.int32)
    if lib().hk_camera_block(st.ctypes.data, W, H, out.ctypes.data, den.ctypes.data, grid.ctypes.data) != 0:
        raise RuntimeError(lib().hk_last_error().decode())
    return {"from": out[0:3].copy(), "llc": out[3:6].copy(), "hor": out[6:9].copy(), "ver": out[9:12].copy(), "den_w": float(den[0]), "den_h": float(den[1]),
            "gw": int(grid[0]), "gh": int(grid[1])}


REPROJECT_DEFAULTS = {"max_history": 32, "normal_cos": 0.9, "plane_tolerance": 0.01, "material_mask": 0xFFFFFFC3, "sky": 1}


def reproject(acc, hist, frames, from_settings13, to_settings13, guides_from, guides_to, nthreads=4, m2=None, **params):
    """dr_accum_reproject on the host (device_reproject.hpp): the accumulator acc (int32[W, H, 3] as dr_accum_read returns it), its history
    plane hist (int32[W, H] or None), the frames added since, both views' settings13 and guides (dicts with "t", "normal", "material" shaped
    like dogeray_amd.Context.render_aov's) -> (acc int32[W, H, 3], hist int32[W, H], counts dict) of the `to` view.  params: the fields of
    dr_reproject_params (the rest default).  m2: the second-moment plane (uint64[W, H]) -- it is carried as well (hk_reproject_m2) and the
    result is (acc, hist, counts, m2 uint64[W, H])."""
    acc = np.ascontiguousarray(acc, dtype=np.int32)
    W, H = acc.shape[0], acc.shape[1]
    a, b = np.ascontiguousarray(from_settings13, dtype=np.float32), np.ascontiguousarray(to_settings13, dtype=np.float32)
    p = dict(REPROJECT_DEFAULTS)
    for k, v in params.items():
        if k not in p:
            raise TypeError("unknown reproject parameter %r" % k)
        p[k] = v
    raw = np.zeros(5, dtype=np.int32)
    raw[0] = p["max_history"]
    raw[1:3] = np.array([p["normal_cos"], p["plane_tolerance"]], np.float32).view(np.int32)
    raw[3] = np.array([p["material_mask"] & 0xFFFFFFFF], np.uint32).view(np.int32)[0]
    raw[4] = p["sky"]
    if hist is not None:
        hist = np.ascontiguousarray(hist, dtype=np.int32)
        assert hist.shape == (W, H)
    g = [np.ascontiguousarray(d[k], dtype=t) for d in (guides_from, guides_to) for k, t in (("t", np.float32), ("normal", np.float32), ("material", np.int32))]
    for k, st in ((0, a), (3, b)):          # each view's guides are its own pixel grid (the call refuses two different grids)
        div = int(st[11]) if np.isfinite(st[11]) and st[11] >= 1 else 1
        gw, gh = W // div // 8 * 8, H // div // 8 * 8
        assert g[k].shape == (gh, gw) and g[k + 1].shape == (gh, gw, 3) and g[k + 2].shape == (gh, gw), "guides are not the %d x %d pixel grid" % (gw, gh)
    out_acc = np.zeros((W, H, 3), np.int32)
    out_hist = np.zeros((W, H), np.int32)
    counts = (C.c_longlong * 5)()
    out_m2 = None
    if m2 is not None:
        m2 = np.ascontiguousarray(m2, dtype=np.uint64)
        assert m2.shape == (W, H)
        out_m2 = np.zeros((W, H), np.uint64)
    rc = lib().hk_reproject_m2(acc.ctypes.data, hist.ctypes.data if hist is not None else None, W, H, int(frames), a.ctypes.data, b.ctypes.data,
                               *[x.ctypes.data for x in g], raw.ctypes.data, out_acc.ctypes.data, out_hist.ctypes.data, C.cast(counts, C.c_void_p), nthreads,
                               m2.ctypes.data if m2 is not None else None, out_m2.ctypes.data if m2 is not None else None)
    if rc != 0:
        raise RuntimeError(lib().hk_last_error().decode())
    cd = dict(zip(("pixels", "valid", "masked", "offscreen", "rejected"), [int(v) for v in counts]))
    return (out_acc, out_hist, cd) if m2 is None else (out_acc, out_hist, cd, out_m2)


def moments_add(acc, m2, frame):
    """The fused add of the second-moment plane on the host (device_moments.hpp): acc int32[W, H, 3] += frame and m2 uint64[W, H] += the frame's
    capped luma x 256, squared (saturating), IN PLACE; both must be C-contiguous arrays of exactly these types."""
    assert acc.dtype == np.int32 and m2.dtype == np.uint64 and acc.flags.c_contiguous and m2.flags.c_contiguous
    frame = np.ascontiguousarray(frame, dtype=np.int32)
    assert acc.shape == frame.shape and acc.shape[-1] == 3 and m2.size * 3 == acc.size
    if lib().hk_moments_add(acc.ctypes.data, frame.ctypes.data, m2.ctypes.data, m2.size) != 0:
        raise RuntimeError(lib().hk_last_error().decode())
    return acc, m2


ERROR_FIELDS = ("estimated", "above", "sum_var_q16")


def error(acc, hist, m2, settings13, divide_by, tolerance, nthreads=4):
    """dr_accum_error on the host (device_moments.hpp): the accumulator acc (int32[W, H, 3]), its history plane hist (int32[W, H] or None) and
    its second-moment plane m2 (uint64[W, H]) -> (sigma float32[H, W], result dict with the fields of dr_error_result)."""
    acc = np.ascontiguousarray(acc, dtype=np.int32)
    W, H = acc.shape[0], acc.shape[1]
    st = np.ascontiguousarray(settings13, dtype=np.float32)
    m2 = np.ascontiguousarray(m2, dtype=np.uint64)
    assert m2.shape == (W, H)
    if hist is not None:
        hist = np.ascontiguousarray(hist, dtype=np.int32)
        assert hist.shape == (W, H)
    sigma = np.zeros((H, W), np.float32)
    res = np.zeros(19, np.uint64)
    grid = np.zeros(2, np.int32)
    rc = lib().hk_error(acc.ctypes.data, hist.ctypes.data if hist is not None else None, m2.ctypes.data, W, H, int(divide_by), float(tolerance),
                        st.ctypes.data, sigma.ctypes.data, res.ctypes.data, grid.ctypes.data, nthreads)
    if rc != 0:
        raise RuntimeError(lib().hk_last_error().decode())
    d = {"pixels": int(grid[0]) * int(grid[1]), "estimated": int(res[0]), "above": int(res[1]), "sum_var_q16": int(res[2]), "bins": [int(v) for v in res[3:]]}
    return sigma, d


BUILD_FIELDS = ("count", "occ", "trav_min", "park_min", "unroll", "wide", "coop", "perframe")
PLAN_FIELDS = BUILD_FIELDS + ("blocks", "log_waves", "clear_wave_log")
CFG_FIELDS = ("traversal", "occupancy", "schedule", "num_cus", "coop_tiles_per_wave", "count")


def _cfg(cfg):
    return (C.c_int * 6)(*[int(cfg[k]) for k in CFG_FIELDS])


def persistent_plan(cfg, work, coop_steps, per_frame, wave_log_on):
    """launch_plan.hpp plan_persistent: cfg is a dict with CFG_FIELDS -> the plan as a tuple of ints in the order of PLAN_FIELDS (the build's
    eight template arguments first)."""
    out = (C.c_int * 11)()
    lib().hk_persistent_plan(_cfg(cfg), int(work), int(coop_steps), int(per_frame), int(wave_log_on), out)
    return tuple(out)


def persistent_can_store_per_frame(cfg):
    return bool(lib().hk_persistent_can_store_per_frame(_cfg(cfg)))


def persistent_builds():
    """The instantiations of render_persistent_kernel (DR_PERSISTENT_BUILDS) as a list of tuples in the order of BUILD_FIELDS."""
    n = lib().hk_persistent_builds(None, 0)
    out = np.zeros((n, 8), np.int32)
    assert lib().hk_persistent_builds(out.ctypes.data, n) == n
    return [tuple(int(v) for v in row) for row in out]


TRACE_PLAN_FIELDS = ("kernel", "traversal", "blocks")


def trace_plan(n, traversal, has_wide, num_cus=256, force=0):
    """launch_plan.hpp plan_trace -> (kernel: 0 one ray per lane / 1 persistent, the traversal really walked, workgroups)"""
    out = (C.c_int * 3)()
    lib().hk_trace_plan(int(n), int(traversal), int(bool(has_wide)), int(num_cus), int(force), out)
    return tuple(out)


def trace_persistent_min_rays():
    return int(lib().hk_trace_persistent_min_rays())


def radiance_plan(n, traversal, has_wide, num_cus=256, force=0):
    """launch_plan.hpp plan_radiance -> (kernel: 0 one ray per lane / 1 persistent, the traversal really walked, workgroups)"""
    out = (C.c_int * 3)()
    lib().hk_radiance_plan(int(n), int(traversal), int(bool(has_wide)), int(num_cus), int(force), out)
    return tuple(out)


def radiance_persistent_min_rays():
    return int(lib().hk_radiance_persistent_min_rays())


def radiance_chunk():
    return int(lib().hk_radiance_chunk())


def radiance_occ():
    return int(lib().hk_radiance_occ())


def radiance_refill_min():
    return int(lib().hk_radiance_refill_min())


def radiance_park():
    return int(lib().hk_radiance_park())


def plan_sky_split(cfg, work, coop_steps, per_frame, wave_log_on):
    """launch_plan.hpp plan_sky_split of persistent_plan's plan for the same arguments: may the launch leave its sky tiles to sky_tiles_kernel"""
    return bool(lib().hk_plan_sky_split(_cfg(cfg), int(work), int(coop_steps), int(per_frame), int(wave_log_on)))


def sky_split(order, region_start, word, regions):
    """device_sky.hpp sky_split_plain (hk_sky_split): order int32[tiles] or None (identity), region_start int32[regions + 1 or more], word uint32[tiles]
    -> (launch_order int32[geometry tiles], launch_region_start int32[17], sky_list int32[sky tiles])."""
    word = np.ascontiguousarray(word, dtype=np.uint32)
    tiles = len(word)
    rs = np.ascontiguousarray(region_start, dtype=np.int32)
    o = np.ascontiguousarray(order, dtype=np.int32) if order is not None else None
    lo, lrs, sky = np.zeros(max(1, tiles), np.int32), np.zeros(17, np.int32), np.zeros(max(1, tiles), np.int32)
    n = lib().hk_sky_split(o.ctypes.data if o is not None else None, rs.ctypes.data, word.ctypes.data, tiles, int(regions), lo.ctypes.data, lrs.ctypes.data,
                           sky.ctypes.data)
    return lo[:tiles - n], lrs, sky[:n]


def sky_units(n_sky, batch, chunk):
    """launch_plan.hpp sky_units: the units (sky tile, chunk of frames) of a launch of `batch` frames with n_sky sky tiles; chunk 0 = the whole batch"""
    return int(lib().hk_sky_units(int(n_sky), int(batch), int(chunk)))


def sky_unit(u, batch, chunk):
    """launch_plan.hpp sky_unit: unit u as (position in sky_list, first frame, frames)"""
    out = (C.c_int * 3)()
    lib().hk_sky_unit(int(u), int(batch), int(chunk), out)
    return int(out[0]), int(out[1]), int(out[2])


def plan_regions(tiles, batch_hint, xcd_regions, short_one_queue, tiles_per_wave, num_cus):
    return int(lib().hk_plan_regions(int(tiles), int(batch_hint), int(xcd_regions), int(short_one_queue), int(tiles_per_wave), int(num_cus)))


def plan_split_limit(num_cus, occupancy, split_parts, split_waves):
    return int(lib().hk_plan_split_limit(int(num_cus), int(occupancy), int(split_parts), int(split_waves)))
