"""ctypes binding of tools/libhostkernel.so: the product's device functions (dogeray_amd/csrc/device_core.hpp) compiled for the host
(tools/host_kernel.cpp and the headers of tools/host_kernel/).  Test and bench infrastructure -- never part of the product library."""
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
_PARTS = os.path.join(_HERE, "host_kernel")
_SOURCES = [os.path.join(_HERE, "host_kernel.cpp")] + [os.path.join(_CSRC, f) for f in ("rts_reader.cpp", "bvh_builder.cpp", "linearise.cpp", "wide_builder.cpp", "capi_host.cpp")]
_lib = None


def build(force=False):
    deps = _SOURCES + [os.path.join(d, f) for d in (_CSRC, _PARTS) for f in os.listdir(d) if f.endswith((".h", ".hpp"))]
    if not force and os.path.exists(_SO) and all(os.path.getmtime(d) <= os.path.getmtime(_SO) for d in deps):
        return _SO
    cxx = "/opt/rocm/lib/llvm/bin/clang++"          # ext_vector_type (u32x4) is a clang extension
    if not os.path.exists(cxx):
        cxx = "clang++"
    # -ffp-contract=off as on the device; -mfma so that the explicit fmaf of the folded node test is one instruction
    cmd = [cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-pthread", "-DDR_HOST_BUILD=1",
           "-I" + _PARTS, "-o", _SO] + _SOURCES
    subprocess.check_call(cmd)
    return _SO


# the constants the device code is built with, each an export without arguments and a function of this module:
# DR_ALLHITS_MAX | rays a wave of the persistent kernel takes from the list per atomic (launch_plan.hpp ALLHITS_CHUNK) | the k of the accuracy bound
# k u (d + 2 Lmax) of nearest_prim (device_nearest.hpp NEAREST_K) | launch_plan.hpp's thresholds and the radiance kernel's shape
_CONSTANTS = (("allhits_max", C.c_int), ("allhits_chunk", C.c_int), ("nearest_k", C.c_int), ("allhits_persistent_min_rays", C.c_longlong),
              ("trace_persistent_min_rays", C.c_longlong), ("radiance_persistent_min_rays", C.c_longlong), ("radiance_chunk", C.c_int), ("radiance_occ", C.c_int),
              ("radiance_refill_min", C.c_int), ("radiance_park", C.c_int))
# every export of the library: (name, restype, argtypes).  An int restype is a status (0, or -1 with hk_last_error) unless the entry's comment says otherwise.
_I, _Q, _F, _D, _P, _U64, _PI = C.c_int, C.c_longlong, C.c_float, C.c_double, C.c_void_p, C.c_uint64, C.POINTER(C.c_int)
_VIEW = [_P, _P, _I, _I]                 # a scene handle, settings13, W, H
_API = [
    ("hk_last_error", C.c_char_p, []),
    ("hk_scene_load", _P, [C.c_char_p, C.c_char_p]),
    ("hk_scene_free", None, [_P]),
    ("hk_has_wide", _I, [_P]),
    ("hk_wide_depth", _I, [_P]),
    ("hk_wide_info", _I, [_P, _I, _P]),
    ("hk_wide_mu", _I, [_P, _P]),
    ("hk_wide_leaves", _Q, [_P, _P, _P, _P, _Q, _Q]),
    ("hk_check_uniform", _Q, [_Q, C.c_ulonglong]),
    ("hk_check_reject", _Q, [_Q, C.c_ulonglong, C.POINTER(_D)]),
    ("hk_ray_margin", None, [_Q, _P, _P, _F, _F, _F, _P]),
    ("hk_ray_margin_k", None, [_Q, _P, _P, _F, _F, _F, _F, _P]),
    ("hk_cert_factor_k", _F, [_D]),
    ("hk_slab", None, [_Q] + [_P] * 5),
    ("hk_lean_pop", None, [_Q] + [_P] * 4),
    ("hk_step_masks", None, [_Q] + [_P] * 5),
    ("hk_tri_hit", None, [_Q] + [_P] * 6),
    ("hk_tri_hit_uv", None, [_Q] + [_P] * 7),
    ("hk_tri_barycentrics", None, [_Q] + [_P] * 6),
    ("hk_hit_inputs", _I, [_Q, _I, _I, _I] + [_P] * 6 + [_I] + [_P] * 8),
    ("hk_cert_check", _I, _VIEW + [_D, _F, _Q, _U64, _P, _P]),
    ("hk_cert_levels", _I, _VIEW + [_I, _I, _F, _Q, _U64, _P, _P]),
    ("hk_camera_entry", _I, _VIEW + [_I, _I, _I, _P, _P]),
    ("hk_camera_entry_check", _I, _VIEW + [_I, _I, _U64, _U64, _I, _I, _P, _P]),
    ("hk_persistent_plan", None, [_PI, _Q, _I, _I, _I, _PI]),
    ("hk_persistent_can_store_per_frame", _I, [_PI]),
    ("hk_persistent_builds", _I, [_P, _I]),
    ("hk_plan_regions", _I, [_I] * 6),
    ("hk_sample_order_magic", C.c_uint, [_I, _I]),
    ("hk_tile_sample", None, [C.c_uint, _I, _I, _PI]),
    ("hk_tile_samples", None, [_I, _I, _PI]),
    ("hk_plan_split_limit", _I, [_I] * 4),
    ("hk_cursor_take", None, [_I, _I, _I, _PI]),
    ("hk_cursor_layout", None, [_PI]),
    ("hk_cursor_ring_blocks", _I, [_I, _I]),
    ("hk_plan_sky_split", _I, [_PI, _Q, _I, _I, _I]),
    ("hk_trace_plan", None, [_Q, _I, _I, _I, _I, _P]),
    ("hk_radiance_plan", None, [_Q, _I, _I, _I, _I, _P]),
    ("hk_allhits_plan", None, [_Q, _I, _I, _I, _P]),
    ("hk_launch_state_new", _P, []),
    ("hk_launch_state_free", None, [_P]),
    ("hk_launch_state_read", None, [_P, _P]),
    ("hk_launch_state_invalidate", None, [_P, _I]),
    ("hk_order_begin", _I, [_P, _P, _P, _I, _I, _I, _I]),
    ("hk_order_end", _I, [_P, _I, _I]),
    ("hk_order_pipeline_refresh", _I, [_P, _P, _P, _I, _I]),
    ("hk_camera_words_plan", _I, [_P, _P, _P, _I, _I, _I, _I, _I, _I]),
    ("hk_camera_words_compute", None, [_P, _P, _P, _I, _I, _I]),
    ("hk_camera_words_readable", _I, [_P]),
    ("hk_sky_split_launch", _I, [_P, _I, _I, _I, _I, _I]),
    ("hk_site_use", _I, [_I, _I]),                            # bits
    ("hk_pipeline_new", _P, []),
    ("hk_pipeline_free", None, [_P]),
    ("hk_pipeline_parked_max", _I, []),                       # the constant
    ("hk_pipeline_group_room", _I, [_I, _I]),                 # frames
    ("hk_pipeline_locate", None, [_P, _U64, _PI]),
    ("hk_pipeline_submit_closes", _I, [_P, _I, _U64]),        # 1 / 0
    ("hk_pipeline_owed_after", _I, [_P, _I]),                 # images
    ("hk_pipeline_submit_overfills", _I, [_P, _I]),           # 1 / 0
    ("hk_pipeline_hold", _U64, [_P, _I, _U64, _I]),
    ("hk_pipeline_group_full", _I, [_P, _I]),                 # 1 / 0
    ("hk_pipeline_flush_size", _I, [_P, _I]),                 # frames
    ("hk_pipeline_drop_held", None, [_P]),
    ("hk_pipeline_group_begin", None, [_P, _I, _P]),
    ("hk_pipeline_group_plan", None, [_P, _I, _I, _PI]),
    ("hk_pipeline_group_take_slot", None, [_P]),
    ("hk_pipeline_group_commit", None, [_P, _P]),
    ("hk_pipeline_mark_waited", _I, [_P, _U64]),              # 1 / 0
    ("hk_pipeline_image", _Q, [_P, _U64]),
    ("hk_pipeline_all_drained", None, [_P]),
    ("hk_pipeline_join", None, [_P, _PI]),
    ("hk_pipeline_restart_numbering", None, [_P, _I]),
    ("hk_pipeline_dump", _I, [_P, _P, _I]),                   # words
    ("hk_sky_split", _I, [_P, _P, _P, _I, _I, _P, _P, _P]),
    ("hk_sky_pixel", _I, _VIEW + [_F, _U64, _U64, _I, _I, _P, _P, _P]),
    ("hk_sky_units", C.c_uint, [C.c_uint, _I, _I]),
    ("hk_sky_unit", None, [C.c_uint, _I, _I, _PI]),
    ("hk_sky_units_render", _Q, _VIEW + [_F, _U64, _U64, _I, _I, _I, _P, _P, _P, _P]),
    ("hk_kat_sample", _I, [_Q] + [_P] * 7),
    ("hk_kat_outside", _I, [_Q, _P, _P]),
    ("hk_kat_tex", _I, [_P, _Q] + [_P] * 4),
    ("hk_kat_bounce", _I, [_P, _Q] + [_P] * 12),
    ("hk_kat_miss", _I, [_P, _Q, _P, _P, _I, _F, _P]),
    ("hk_kat_camera", _I, [_P, _I, _I, _U64, C.c_uint32, _Q] + [_P] * 6),
    ("hk_kat_store", _I, [_Q, _P, _I, _P]),
    ("hk_hit", _I, [_P, _I, _I, _Q] + [_P] * 5),
    ("hk_trace", _I, [_P, _I, _I, _I, _Q] + [_P] * 8),
    ("hk_ray_surface", _I, [_P, _I, _Q] + [_P] * 9),
    ("hk_radiance", _I, [_P, _I, _I, _Q] + [_P] * 4 + [_I, _I, _F, _I, _U64, _P, _P]),
    ("hk_allhits", _I, [_P, _I, _I, _Q] + [_P] * 3 + [_I] * 3 + [_P] * 9 + [_I]),
    ("hk_allhits_brute", _I, [_P, _Q] + [_P] * 3 + [_I] * 2 + [_P] * 3 + [_I]),
    ("hk_nearest", _I, [_P, _I, _I, _Q] + [_P] * 9 + [_I]),
    ("hk_nearest_brute", _I, [_P, _Q] + [_P] * 8 + [_I]),
    ("hk_nearest_prim", None, [_Q] + [_P] * 8),
    ("hk_nearest_prims", _Q, [_P] * 8),
    ("hk_nearest_records", _Q, [_P, _I, _I]),
    ("hk_render", _I, _VIEW + [_F, _U64, _I, _I, _I, _I, _P, _P, _P, _I, _I, _P]),
    ("hk_aov", _I, _VIEW + [_I] * 6 + [_P] * 9),
    ("hk_aov_lens", _I, _VIEW + [_I] * 4 + [_U64, _U64] + [_I] * 4 + [_P] * 6),
    ("hk_denoise", _I, [_P, _I, _I, _I] + [_P] * 8 + [_I, _P, _P]),
    ("hk_upscale", _I, [_P, _I, _I, _I] + [_P] * 14 + [_I, _P, _P]),
    ("hk_camera_block", _I, [_P, _I, _I, _P, _P, _P]),
    ("hk_reproject", _I, [_P, _P, _I, _I, _I] + [_P] * 12 + [_I, _P, _P]),
    ("hk_moments_add", _I, [_P, _P, _P, _Q]),
    ("hk_error", _I, [_P, _P, _P, _I, _I, _I, _F, _P, _P, _P, _P, _I]),
    ("hk_adaptive_select", _I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    ("hk_subset_split", _I, [_P, _P, _P, _I, _I, _P, _P]),    # flagged tiles
    ("hk_adaptive_add", _I, [_P, _P, _P, _I, _I, _P, _P, _I, _P, _I]),
] + [("hk_" + k, t, []) for k, t in _CONSTANTS]
API_SYMBOLS = [a[0] for a in _API]


def bind(cdll):
    """the table applied to a loaded libhostkernel.so (this tree's or another build of it); returns cdll"""
    for name, res, args in _API:
        f = getattr(cdll, name)
        f.restype, f.argtypes = res, args
    return cdll


def lib():
    global _lib
    if _lib is None:
        _lib = bind(C.CDLL(build()))
    return _lib


def _ok(rc):
    if rc != 0:
        raise RuntimeError(lib().hk_last_error().decode())


def _arr(a, dtype, shape=None):
    """a as a C-contiguous array of dtype, of `shape` where one is given; None stays None"""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    assert shape is None or a.shape == shape, "an array of shape %r where %r is expected" % (a.shape, shape)
    return a


def _f32(*arrays):
    return [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]


def _ptr(a):
    """the address of an array; None for None"""
    return None if a is None else a.ctypes.data


def _rays(o, d, tmax=None):
    """rays as (o float32[n, 3], d float32[n, 3], tmax float32[n] or None, n); points with radii take the same path (d None)"""
    o = _arr(o, np.float32)
    n = o.shape[0]
    assert o.shape == (n, 3)
    return o, _arr(d, np.float32, (n, 3)), _arr(tmax, np.float32, (n,)), n


# the channels the queries return: dtype and width -- 0 one value per ray, 1 one per entry (ray, point, pixel, or list entry), w > 1 a vector per entry
_CHANNELS = {"count": (np.int32, 0), "occluded": (np.int32, 1), "bounces": (np.int32, 1), "object": (np.int32, 1), "material": (np.int32, 1),
             "t": (np.float32, 1), "distance": (np.float32, 1), "d2": (np.float32, 1), "depth": (np.float32, 1), "coverage": (np.float32, 1), "uv": (np.float32, 2),
             "normal": (np.float32, 3), "albedo": (np.float32, 3), "point": (np.float32, 3), "dir": (np.float32, 3), "radiance": (np.float32, 3)}
NEAREST_CHANNELS = ("distance", "d2", "object", "material", "point", "uv")      # in the order of dr_nearest_buffers
ALLHITS_CHANNELS = ("count", "t", "object", "material", "distance", "normal", "uv", "albedo")      # in the order of dr_allhits_buffers
_SURFACE_CHANNELS = ("material", "distance", "normal", "uv", "albedo")          # what hk_ray_surface writes
_AOV_CHANNELS = ("t", "distance", "depth", "object", "material", "normal", "uv", "albedo", "dir")
_AOV_LENS_CHANNELS = ("coverage", "depth", "distance", "material", "normal", "albedo")      # in the order of dr_aov_lens_buffers


def _channels(lead, names, K=None):
    """zeroed arrays {name: array} for `names`: shape lead (a tuple), then K where the channel has list entries, then the channel's width"""
    shape = lambda w: lead + ((K,) if K is not None and w > 0 else ()) + ((w,) if w > 1 else ())
    return {k: np.zeros(shape(_CHANNELS[k][1]), _CHANNELS[k][0]) for k in names}


def _ptrs(out, order):
    """the addresses of the dict's arrays in the library's order, None for the channels not asked for"""
    return [_ptr(out.get(k)) for k in order]


def _u64(v):
    return int(v) & (2 ** 64 - 1)


def _div(st):
    """the resolution divisor of settings13 as the library reads it"""
    return int(st[11]) if np.isfinite(st[11]) and st[11] >= 1 else 1


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
    return _kat("camera", (x, y, sample), head=(st.ctypes.data, int(W), int(H), _u64(frame_seed), int(stride) & 0xFFFFFFFF))


def kat_store(color, spp):
    return _kat("store", (color,), mid=(int(spp),))[0]


def slab(o, d, mn, mx):
    """device_intersect.hpp slab() on n ray / box pairs (hk_slab): int32[n], 1 where the ray enters the box"""
    o, d, mn, mx = _f32(o, d, mn, mx)
    hit = np.zeros(o.shape[0], np.int32)
    lib().hk_slab(o.shape[0], *map(_ptr, (o, d, mn, mx, hit)))
    return hit


def lean_pop(top, sp, stack):
    """device_wide.hpp wide_pop and wide_pop_lean on n stack states (hk_lean_pop): top uint32[n], sp int32[n] in 0 .. 16, stack uint32[n, 16] (the
    lane's stack words) -> (int32[n, 3], int32[n, 3]): next record, remaining word, stack pointer after wide_pop and after wide_pop_lean"""
    top, sp, stack = _arr(top, np.uint32), _arr(sp, np.int32), _arr(stack, np.uint32)
    n = top.shape[0]
    assert sp.shape == (n,) and stack.shape == (n, 16) and sp.min() >= 0 and sp.max() <= 16
    out = np.zeros((n, 2, 3), np.int32)
    lib().hk_lean_pop(n, *map(_ptr, (top, sp, stack, out)))
    return out[:, 0], out[:, 1]


def step_masks(node, draining, leaf_min, exclusive):
    """device_walk.hpp step_masks on n waves (hk_step_masks): node int32[n, 64] (each lane's link or LANE_* state), draining / leaf_min / exclusive
    int32[n] -> (uint64[n], uint64[n]): the lanes that take the step, and those of them that take it as leaves"""
    node, draining, leaf_min, exclusive = (_arr(a, np.int32) for a in (node, draining, leaf_min, exclusive))
    n = node.shape[0]
    assert node.shape == (n, 64) and draining.shape == leaf_min.shape == exclusive.shape == (n,)
    out = np.zeros((n, 2), np.uint64)
    lib().hk_step_masks(n, *map(_ptr, (node, draining, leaf_min, exclusive, out)))
    return out[:, 0].copy(), out[:, 1].copy()


def tri_hit_uv(o, d, v0, e1, e2):
    """device_intersect.hpp tri_hit in both forms on n ray / triangle pairs -> (t of the plain form, t and uv float32[n, 2] of the form that hands out
    the barycentrics)"""
    ins = _f32(o, d, v0, e1, e2)
    n = ins[0].shape[0]
    t0, t1, uv = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros((n, 2), np.float32)
    lib().hk_tri_hit(n, *map(_ptr, ins + [t0]))
    lib().hk_tri_hit_uv(n, *map(_ptr, ins + [t1, uv]))
    return t0, t1, uv


def tri_barycentrics(o, d, v0, e1, e2):
    """device_surface.hpp tri_barycentrics on n ray / triangle pairs -> float32[n, 2]: ux, uy as surface_normal forms them"""
    ins = _f32(o, d, v0, e1, e2)
    uv = np.zeros((ins[0].shape[0], 2), np.float32)
    lib().hk_tri_barycentrics(ins[0].shape[0], *map(_ptr, ins + [uv]))
    return uv


def hit_inputs(o, d, t, uv, prims, shade, seed, form=0, carried=False, lazy=False, tex=None, texels=None):
    """hk_hit_inputs: what the shade phase forms at n hits.  prims uint32[n, 12] (DevPrim words), shade uint32[n, 32] (DevShade words), tex int32[k, 4]
    (DevTex words) with texels uint32[...]; form 0 = shade_prepare, form 1 = shade_prepare_hit<carried, lazy> -> dict of alive int32[n],
    texco float32[n, 2], sc uint32[n, 16] (the words of ShadeCtx), emitted float32[n, 3], next uint32[n, 2]."""
    o, d, t, uv = _f32(o, d, t, uv)
    prims, shade, seed = _arr(prims, np.uint32), _arr(shade, np.uint32), _arr(seed, np.uint64)
    n = o.shape[0]
    assert prims.shape == (n, 12) and shade.shape == (n, 32) and uv.shape == (n, 2) and t.shape == (n,) and seed.shape == (n,)
    tex = _arr(tex if tex is not None else np.zeros((1, 4)), np.int32)
    texels = _arr(texels if texels is not None else np.zeros(1), np.uint32)
    out = {"alive": np.zeros(n, np.int32), "texco": np.zeros((n, 2), np.float32), "sc": np.zeros((n, 16), np.uint32), "emitted": np.zeros((n, 3), np.float32),
           "next": np.zeros((n, 2), np.uint32)}
    _ok(lib().hk_hit_inputs(n, int(form), int(bool(carried)), int(bool(lazy)), *map(_ptr, (o, d, t, uv, prims, shade)), int(tex.shape[0]) if texels.size > 1 else 0,
                            *map(_ptr, (tex, texels, seed)), *_ptrs(out, ("alive", "texco", "sc", "emitted", "next"))))
    return out


globals().update({k: (lambda k=k: int(getattr(lib(), "hk_" + k)())) for k, _ in _CONSTANTS})      # allhits_max() .. radiance_park()


def nearest_prim(kind, a, b, c, p):
    """nearest_prim (device_nearest.hpp) pair by pair -> (d2 [n], q [n, 3], uv [n, 2])"""
    ins = [_arr(kind, np.int32)] + _f32(a, b, c, p)
    n = len(ins[0])
    d2, q, uv = np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 2), np.float32)
    lib().hk_nearest_prim(n, *map(_ptr, ins + [d2, q, uv]))
    return d2, q, uv


class Scene:
    def __init__(self, rts_path, texdir=""):
        self.h = lib().hk_scene_load(os.fsencode(rts_path), os.fsencode(texdir or ""))
        _ok(0 if self.h else -1)

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
        o, d, _, n = _rays(o, d)
        t, idx = np.zeros(n, np.float32), np.zeros(n, np.int32)
        vis = np.zeros(n, np.int32) if want_visits else None
        _ok(lib().hk_hit(self.h, int(traversal), int(tree), n, *map(_ptr, (o, d, t, idx, vis))))
        return (t, idx, vis) if want_visits else (t, idx)

    def trace(self, o, d, tmax=None, traversal=2, tree=2, any_hit=False, channels=("t", "object"), want_visits=False):
        """dr_trace_rays on the host (hk_trace, hk_ray_surface): the rays (o, d[, tmax]) by the walks of device_trace.hpp -> a dict of arrays as
        dogeray_amd.Context.trace returns it ({"occluded"} for any_hit); want_visits adds "visits", the boxes tested per ray."""
        o, d, tmax, n = _rays(o, d, tmax)
        t, idx, slot, occ, vis = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        _ok(lib().hk_trace(self.h, int(traversal), int(tree), 1 if any_hit else 0, n, *map(_ptr, (o, d, tmax, t, idx, occ, slot, vis))))
        if any_hit:
            out = {"occluded": occ}
        else:
            extra = _channels((n,), [k for k in channels if k in _SURFACE_CHANNELS])
            if extra:
                _ok(lib().hk_ray_surface(self.h, int(tree), n, *map(_ptr, (o, d, t, slot)), *_ptrs(extra, _SURFACE_CHANNELS)))
            out = {k: t if k == "t" else idx if k == "object" else extra[k] for k in channels}
        if want_visits:
            out["visits"] = vis
        return out

    def radiance(self, o, d, spp=1, max_depth=10, background=1.0, backtex=-1, seed=0, seeds=None, skip=None, traversal=2, tree=2,
                 channels=("radiance", "bounces")):
        """dr_trace_radiance on the host (hk_radiance: device_radiance.hpp radiance_ray over the host walks): the arguments and the dict of
        dogeray_amd.Context.radiance, by the walk of `traversal` over the tree of wide_tree = `tree`."""
        o, d, _, n = _rays(o, d)
        seeds, skip = _arr(seeds, np.uint64, (n,)), _arr(skip, np.int32, (n,))
        out = _channels((n,), channels)
        _ok(lib().hk_radiance(self.h, int(traversal), int(tree), n, *map(_ptr, (o, d, seeds, skip)), int(spp), int(max_depth), float(background), int(backtex),
                              _u64(seed), *_ptrs(out, ("radiance", "bounces"))))
        return out

    def nearest(self, p, rmax=None, walk=2, tree=2, channels=NEAREST_CHANNELS, want_visits=False, nthreads=1):
        """dr_query_nearest on the host (hk_nearest): the points p[, rmax] by the walks of device_nearest.hpp -- walk 2 the 4-way records of the tree of
        wide_tree = `tree`, 0 the threaded links -> a dict of arrays as dogeray_amd.Context.nearest returns it; want_visits adds "visits", the records
        visited per query."""
        p, _, rmax, n = _rays(p, None, rmax)
        out = _channels((n,), channels)
        vis = np.zeros(n, np.int32)
        _ok(lib().hk_nearest(self.h, int(walk), int(tree), n, _ptr(p), _ptr(rmax), *_ptrs(out, NEAREST_CHANNELS), _ptr(vis), int(nthreads)))
        if want_visits:
            out["visits"] = vis
        return out

    def nearest_brute(self, p, rmax=None, channels=NEAREST_CHANNELS, nthreads=1):
        """the same answer by its definition (hk_nearest_brute): the key-minimum of nearest_prim over every primitive, no tree"""
        p, _, rmax, n = _rays(p, None, rmax)
        out = _channels((n,), channels)
        _ok(lib().hk_nearest_brute(self.h, n, _ptr(p), _ptr(rmax), *_ptrs(out, NEAREST_CHANNELS), int(nthreads)))
        return out

    def nearest_prims(self):
        """the primitive records in slot order: dict kind (0 sphere, 1 triangle, 2 none), a, b, c [n, 3], orig, material, and lmax (the pruning slack's scene constant)"""
        n = int(lib().hk_nearest_prims(self.h, *([None] * 7)))
        kind, orig, mat = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        a, b, c = (np.zeros((n, 3), np.float32) for _ in range(3))
        lmax = np.zeros(1, np.float32)
        lib().hk_nearest_prims(self.h, *map(_ptr, (kind, a, b, c, orig, mat, lmax)))
        return {"kind": kind, "a": a, "b": b, "c": c, "orig": orig, "material": mat, "lmax": float(lmax[0])}

    def nearest_records(self, walk=2, tree=2):
        """records of the walk Scene.nearest takes"""
        return int(lib().hk_nearest_records(self.h, int(walk), int(tree)))

    def allhits(self, o, d, tmax=None, max_hits=4, kind_mask=3, walk=2, tree=2, channels=("count", "t", "object"), zero_margin=False, want_visits=False,
                nthreads=1):
        """dr_trace_all_hits on the host (hk_allhits): the rays (o, d[, tmax]) by the walks of device_allhits.hpp -- walk 2 the 4-way records of the tree
        of wide_tree = `tree`, 0 the threaded links -> a dict of arrays as dogeray_amd.Context.trace_all returns it; zero_margin forces the wide node
        step's margins to zero (the switch of tests/test_allhits_host.py); want_visits adds "visits", the records visited per ray."""
        o, d, tmax, n = _rays(o, d, tmax)
        out = _channels((n,), channels, max(int(max_hits), 0))      # (a list length out of range is refused by the library)
        vis = np.zeros(n, np.int32)
        _ok(lib().hk_allhits(self.h, int(walk), int(tree), n, _ptr(o), _ptr(d), _ptr(tmax), int(max_hits), int(kind_mask), int(bool(zero_margin)),
                             *_ptrs(out, ALLHITS_CHANNELS), _ptr(vis), int(nthreads)))
        if want_visits:
            out["visits"] = vis
        return out

    def allhits_brute(self, o, d, tmax=None, max_hits=4, kind_mask=3, nthreads=1):
        """the same answer by its definition (hk_allhits_brute): a loop over every leaf record, no walk -> {"count", "t", "object"}"""
        o, d, tmax, n = _rays(o, d, tmax)
        out = _channels((n,), ("count", "t", "object"), max(int(max_hits), 0))
        _ok(lib().hk_allhits_brute(self.h, n, _ptr(o), _ptr(d), _ptr(tmax), int(max_hits), int(kind_mask), *_ptrs(out, ("count", "t", "object")), int(nthreads)))
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
        _ok(lib().hk_wide_info(self.h, int(tree), out.ctypes.data))
        return {"wide_depth": int(out[0]), "wide_own_bounds": int(out[1]), "wide_nodes": int(out[2])}

    def render(self, settings13, W, H, background, frame_seed, traversal=2, nthreads=1, col_mod=1, col_rem=0, count=True, level_plane=None, cert_factor=40,
               graded=1, entry_plane=None):
        """One frame: (int32[W, H, 3] indexed [x, y], counters dict or None).  level_plane: the grades of the view's grazing certificate
        (cert_levels()[0] for the same cert_factor / graded) -- the frame is rendered over the default tree with the camera rays' certified margins.
        entry_plane: the entry codes of the view's camera rays (camera_entry()[0] for the same stripe): they start their walks there."""
        st, plane, eplane = _arr(settings13, np.float32), _arr(level_plane, np.uint8), _arr(entry_plane, np.int32)
        out = np.zeros((W, H, 3), dtype=np.int32)
        ctr = (C.c_uint64 * 6)()
        _ok(lib().hk_render(self.h, st.ctypes.data, W, H, float(background), _u64(frame_seed), traversal, nthreads, col_mod, col_rem, out.ctypes.data,
                            C.cast(ctr, C.c_void_p) if count else None, _ptr(plane), int(cert_factor), int(graded), _ptr(eplane)))
        return out, (dict(zip(("rays", "V", "L", "S", "T", "samples"), [int(v) for v in ctr])) if count else None)

    def camera_entry(self, settings13, W, H, col_mod=1, col_rem=0, mutant=0):
        """The camera rays' entry table of a view on the host (hk_camera_entry): (int32 entry codes, a word per tile of the stripe, and a dict of counts),
        or None when the view or the scene gives no table.  mutant: one of device_cert.hpp's wrong rules (1 rect narrowed, 2 no lens term, 3 highest
        rank off by one, 4 no entry for a tile with one leaf)."""
        st = _arr(settings13, np.float32)
        gx, gy = W // _div(st) // 8, H // _div(st) // 8
        ncols = (gx - col_rem + col_mod - 1) // col_mod if gx > col_rem else 0
        codes = np.zeros(max(1, ncols * gy), np.int32)
        out = np.zeros(32, np.int64)
        rc = lib().hk_camera_entry(self.h, st.ctypes.data, W, H, int(col_mod), int(col_rem), int(mutant), codes.ctypes.data, out.ctypes.data)
        if rc > 0:
            return None
        _ok(rc)
        assert int(out[0]) == ncols * gy
        return codes[:ncols * gy], {"tiles": int(out[0]), "none": int(out[1]), "root": int(out[2]), "leaf": int(out[3]), "every": int(out[4]), "leaves": int(out[5]),
                                    "depth": [int(v) for v in out[8:26]]}

    def camera_entry_check(self, settings13, W, H, codes, seed, stride, frames, col_mod=1, col_rem=0, nthreads=8):
        """hk_camera_entry_check: the kernel's camera rays of `frames` frames against every leaf, by brute force -> dict rays, entered, outside (leaves
        entered that do not lie under their tile's entry: must be 0), entered_below_root."""
        st, codes = _arr(settings13, np.float32), _arr(codes, np.int32)
        out = np.zeros(4, np.int64)
        _ok(lib().hk_camera_entry_check(self.h, st.ctypes.data, W, H, int(col_mod), int(col_rem), int(seed), int(stride), int(frames), int(nthreads),
                                        codes.ctypes.data, out.ctypes.data))
        return {"rays": int(out[0]), "entered": int(out[1]), "outside": int(out[2]), "entered_below_root": int(out[3])}

    def sky_pixel(self, settings13, W, H, background, seed, stride, frames, xs, ys):
        """device_sky.hpp sky_pixel for the pixels (xs, ys), summed over `frames` frames of a launch with dr_render_accumulate's seed and stride
        (hk_sky_pixel): int32[n, 3], what those frames add to the accumulator when every path of the pixels misses."""
        st, xs, ys = _arr(settings13, np.float32), _arr(xs, np.int32), _arr(ys, np.int32)
        out = np.zeros((len(xs), 3), np.int32)
        _ok(lib().hk_sky_pixel(self.h, st.ctypes.data, W, H, float(background), _u64(seed), _u64(stride), int(frames), len(xs), xs.ctypes.data, ys.ctypes.data,
                               out.ctypes.data))
        return out

    def sky_units_render(self, settings13, W, H, background, seed, stride, batch, chunk, sky_list, perm=None, cost=None):
        """device_sky.hpp sky_tile_frames over every unit of a launch of `batch` frames whose sky tiles are sky_list (hk_sky_units_render), the units in
        the order perm gives: (int32[W, H, 3] what the units add to an accumulator of zeros, units run).  cost: uint32[tiles * 64], written in place."""
        st, sl, pm = _arr(settings13, np.float32), _arr(sky_list, np.int32), _arr(perm, np.uint32)
        acc = np.zeros((W, H, 3), np.int32)
        n = lib().hk_sky_units_render(self.h, st.ctypes.data, W, H, float(background), _u64(seed), _u64(stride), int(batch), int(chunk), len(sl), sl.ctypes.data,
                                      _ptr(pm), acc.ctypes.data, _ptr(cost))
        _ok(min(n, 0))
        return acc, int(n)

    def wide_leaves(self):
        """The default tree's leaves in depth-first order: (uint32 record per rank, float32 (n, 6) box per rank -- mn, mx of the record --, uint32 (records, 2)
        rank range per record)."""
        n = int(lib().hk_wide_leaves(self.h, None, None, None, 0, 0))
        _ok(min(n, 0))
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
        st = _arr(settings13, np.float32)
        plane = np.zeros((W // _div(st) // 8) * (H // _div(st) // 8), np.uint8)
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
        st = _arr(settings13, np.float32)
        if window is None:
            div = int(st[11])
            window = (0, 0, W // div // 8 * 8, H // div // 8 * 8)
        x0, y0, w, h = (int(v) for v in window)
        out = _channels((h, w), _AOV_CHANNELS)
        _ok(lib().hk_aov(self.h, st.ctypes.data, W, H, x0, y0, w, h, traversal, nthreads, *_ptrs(out, _AOV_CHANNELS)))
        return out

    def aov_lens(self, settings13, W, H, frame_seed, seed_stride, nframes, window=None, as_guides=False, traversal=2, nthreads=4):
        """dr_render_aov_lens on the host (device_aov_lens.hpp aov_lens_pixel, the nested loop): every channel of the window as a dict of arrays
        shaped like dogeray_amd.Context.render_aov_lens's.  as_guides: the form option guide_frames = nframes hands the denoiser and the upscaler
        (with frame_seed = dogeray_amd.GUIDE_SEED, seed_stride = 1) -- "normal", "albedo", "depth", "material" then go into denoise() / upscale()
        where hk.aov's would."""
        st = _arr(settings13, np.float32)
        if window is None:
            window = (0, 0, W // _div(st) // 8 * 8, H // _div(st) // 8 * 8)
        x0, y0, w, h = (int(v) for v in window)
        out = _channels((h, w), _AOV_LENS_CHANNELS)
        _ok(lib().hk_aov_lens(self.h, st.ctypes.data, W, H, x0, y0, w, h, _u64(frame_seed), _u64(seed_stride), int(nframes), int(bool(as_guides)),
                              traversal, nthreads, *_ptrs(out, _AOV_LENS_CHANNELS)))
        return out


def _params(defaults, given, what):
    """the defaults of a parameter struct with the caller's fields over them"""
    p = dict(defaults)
    for k, v in dict(given).items():
        if k not in p:
            raise TypeError("unknown %s parameter %r" % (what, k))
        p[k] = v
    return p


def _f32_bits(*values):
    return np.array(values, np.float32).view(np.int32)


_GUIDES = (("normal", np.float32), ("albedo", np.float32), ("depth", np.float32), ("material", np.int32))
DENOISE_DEFAULTS = {"iterations": 5, "sigma_luminance": 4.0, "normal_power_log2": 7, "sigma_depth": 1.0, "demodulate": 1, "material_stop": 1}


def _denoise_raw(p):
    """the words of a dr_denoise_params"""
    return np.array([p["iterations"], _f32_bits(p["sigma_luminance"])[0], p["normal_power_log2"], _f32_bits(p["sigma_depth"])[0], p["demodulate"],
                     p["material_stop"]], dtype=np.int32)


def denoise(acc, settings13, divide_by, normal, albedo, depth, material, nthreads=4, hist=None, m2=None, **params):
    """dr_accum_denoise on the host (device_denoise.hpp): the accumulator acc (int32[W, H, 3], column-major as dr_accum_read returns it) and the
    guides as arrays shaped like dogeray_amd.Context.render_aov's (normal / albedo [gh, gw, 3], depth / material [gh, gw]) -> (f32[H, W, 3],
    uint8[H, W, 3]) in dr_accum_present's layout.  hist: the accumulator's history plane (int32[W, H], dr_accum_history_read) -- pixel p then
    divides by hist[p] + divide_by.  m2: the second-moment plane (uint64[W, H], dr_accum_moments_read) -- option "denoise_variance" = 1: pixels with
    four samples or more take their variance from it.  params: the fields of dr_denoise_params (the rest default)."""
    acc = _arr(acc, np.int32)
    W, H = acc.shape[0], acc.shape[1]
    st = _arr(settings13, np.float32)
    raw = _denoise_raw(_params(DENOISE_DEFAULTS, params, "denoise"))
    guides = [_arr(a, t) for a, (_, t) in zip((normal, albedo, depth, material), _GUIDES)]
    f32, rgb = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.uint8)
    hist, m2 = _arr(hist, np.int32, (W, H)), _arr(m2, np.uint64, (W, H))
    _ok(lib().hk_denoise(acc.ctypes.data, W, H, int(divide_by), st.ctypes.data, *map(_ptr, guides), raw.ctypes.data, f32.ctypes.data, rgb.ctypes.data,
                         nthreads, _ptr(hist), _ptr(m2)))
    return f32, rgb


UPSCALE_DEFAULTS = {"mode": 1, "normal_power_log2": 5, "sigma_depth": 1.0, "demodulate": 1, "material_stop": 1}


def upscale(acc, settings13, divide_by, low_guides, full_guides, hist=None, m2=None, prefilter=None, nthreads=4, **params):
    """dr_accum_upscale on the host (device_upscale.hpp): the accumulator acc (int32[W, H, 3] as dr_accum_read returns it), the guides of
    settings13 (low_guides) and of settings13 with element 11 = 1 (full_guides) as dicts with "normal", "albedo", "depth", "material" shaped like
    dogeray_amd.Context.render_aov's (block mode reads neither: both may be None) -> (f32[H, W, 3], uint8[H, W, 3], no-tap mask bool[H, W]) in
    dr_accum_present's layout.  hist / m2 as denoise(); prefilter: None, or a dict of dr_denoise_params fields (the rest default) -- the
    denoiser's host passes run on the low grid first; params: the fields of dr_upscale_params (the rest default)."""
    acc = _arr(acc, np.int32)
    W, H = acc.shape[0], acc.shape[1]
    st = _arr(settings13, np.float32)
    p = _params(UPSCALE_DEFAULTS, params, "upscale")
    raw = np.array([p["mode"], p["normal_power_log2"], _f32_bits(p["sigma_depth"])[0], p["demodulate"], p["material_stop"]], dtype=np.int32)
    pre = None if prefilter is None else _denoise_raw(_params(DENOISE_DEFAULTS, prefilter, "denoise"))

    def guides(g, shape):
        if g is None:
            return [None] * 4
        arrays = [_arr(g[k], t) for k, t in _GUIDES]
        for a in arrays:
            assert a.shape[:2] == shape, "guides are not the %d x %d pixel grid" % (shape[1], shape[0])
        return arrays
    low = guides(low_guides, (H // _div(st) // 8 * 8, W // _div(st) // 8 * 8))
    full = guides(full_guides, (H // 8 * 8, W // 8 * 8))
    f32, rgb, notap = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.uint8), np.zeros((H, W), np.uint8)
    hist, m2 = _arr(hist, np.int32, (W, H)), _arr(m2, np.uint64, (W, H))
    _ok(lib().hk_upscale(acc.ctypes.data, W, H, int(divide_by), st.ctypes.data, *map(_ptr, low + full), raw.ctypes.data, _ptr(pre), f32.ctypes.data,
                         rgb.ctypes.data, notap.ctypes.data, nthreads, _ptr(hist), _ptr(m2)))
    return f32, rgb, notap.astype(bool)


def camera_block(settings13, W, H):
    """The float camera block of a view as the library forms it from settings13 (params_host.hpp fill_view_params): a dict with float32
    "from", "llc", "hor", "ver", float64 "den_w", "den_h" and the pixel grid "gw", "gh"."""
    st = _arr(settings13, np.float32)
    out, den, grid = np.zeros(12, np.float32), np.zeros(2, np.float64), np.zeros(2, np.int32)
    _ok(lib().hk_camera_block(st.ctypes.data, W, H, out.ctypes.data, den.ctypes.data, grid.ctypes.data))
    return {"from": out[0:3].copy(), "llc": out[3:6].copy(), "hor": out[6:9].copy(), "ver": out[9:12].copy(), "den_w": float(den[0]), "den_h": float(den[1]),
            "gw": int(grid[0]), "gh": int(grid[1])}


REPROJECT_DEFAULTS = {"max_history": 32, "normal_cos": 0.9, "plane_tolerance": 0.01, "material_mask": 0xFFFFFFC3, "sky": 1}


def reproject(acc, hist, frames, from_settings13, to_settings13, guides_from, guides_to, nthreads=4, m2=None, **params):
    """dr_accum_reproject on the host (device_reproject.hpp): the accumulator acc (int32[W, H, 3] as dr_accum_read returns it), its history
    plane hist (int32[W, H] or None), the frames added since, both views' settings13 and guides (dicts with "t", "normal", "material" shaped
    like dogeray_amd.Context.render_aov's) -> (acc int32[W, H, 3], hist int32[W, H], counts dict) of the `to` view.  params: the fields of
    dr_reproject_params (the rest default).  m2: the second-moment plane (uint64[W, H]) -- it is carried as well and the result is
    (acc, hist, counts, m2 uint64[W, H])."""
    acc = _arr(acc, np.int32)
    W, H = acc.shape[0], acc.shape[1]
    a, b = _arr(from_settings13, np.float32), _arr(to_settings13, np.float32)
    p = _params(REPROJECT_DEFAULTS, params, "reproject")
    raw = np.zeros(5, dtype=np.int32)
    raw[0] = p["max_history"]
    raw[1:3] = _f32_bits(p["normal_cos"], p["plane_tolerance"])
    raw[3] = np.array([p["material_mask"] & 0xFFFFFFFF], np.uint32).view(np.int32)[0]
    raw[4] = p["sky"]
    hist, m2 = _arr(hist, np.int32, (W, H)), _arr(m2, np.uint64, (W, H))
    g = [_arr(d[k], t) for d in (guides_from, guides_to) for k, t in (("t", np.float32), ("normal", np.float32), ("material", np.int32))]
    for k, st in ((0, a), (3, b)):          # each view's guides are its own pixel grid (the call refuses two different grids)
        gw, gh = W // _div(st) // 8 * 8, H // _div(st) // 8 * 8
        assert g[k].shape == (gh, gw) and g[k + 1].shape == (gh, gw, 3) and g[k + 2].shape == (gh, gw), "guides are not the %d x %d pixel grid" % (gw, gh)
    out_acc, out_hist = np.zeros((W, H, 3), np.int32), np.zeros((W, H), np.int32)
    out_m2 = None if m2 is None else np.zeros((W, H), np.uint64)
    counts = (C.c_longlong * 5)()
    _ok(lib().hk_reproject(acc.ctypes.data, _ptr(hist), W, H, int(frames), a.ctypes.data, b.ctypes.data, *map(_ptr, g), raw.ctypes.data, out_acc.ctypes.data,
                           out_hist.ctypes.data, C.cast(counts, C.c_void_p), nthreads, _ptr(m2), _ptr(out_m2)))
    cd = dict(zip(("pixels", "valid", "masked", "offscreen", "rejected"), [int(v) for v in counts]))
    return (out_acc, out_hist, cd) if m2 is None else (out_acc, out_hist, cd, out_m2)


def moments_add(acc, m2, frame):
    """The fused add of the second-moment plane on the host (device_moments.hpp): acc int32[W, H, 3] += frame and m2 uint64[W, H] += the frame's
    capped luma x 256, squared (saturating), IN PLACE; both must be C-contiguous arrays of exactly these types."""
    assert acc.dtype == np.int32 and m2.dtype == np.uint64 and acc.flags.c_contiguous and m2.flags.c_contiguous
    frame = _arr(frame, np.int32)
    assert acc.shape == frame.shape and acc.shape[-1] == 3 and m2.size * 3 == acc.size
    _ok(lib().hk_moments_add(acc.ctypes.data, frame.ctypes.data, m2.ctypes.data, m2.size))
    return acc, m2


ERROR_FIELDS = ("estimated", "above", "sum_var_q16")


def error(acc, hist, m2, settings13, divide_by, tolerance, nthreads=4):
    """dr_accum_error on the host (device_moments.hpp): the accumulator acc (int32[W, H, 3]), its history plane hist (int32[W, H] or None) and
    its second-moment plane m2 (uint64[W, H]) -> (sigma float32[H, W], result dict with the fields of dr_error_result)."""
    acc = _arr(acc, np.int32)
    W, H = acc.shape[0], acc.shape[1]
    st, m2, hist = _arr(settings13, np.float32), _arr(m2, np.uint64, (W, H)), _arr(hist, np.int32, (W, H))
    sigma, res, grid = np.zeros((H, W), np.float32), np.zeros(19, np.uint64), np.zeros(2, np.int32)
    _ok(lib().hk_error(acc.ctypes.data, _ptr(hist), m2.ctypes.data, W, H, int(divide_by), float(tolerance), st.ctypes.data, sigma.ctypes.data, res.ctypes.data,
                       grid.ctypes.data, nthreads))
    d = {"pixels": int(grid[0]) * int(grid[1]), "estimated": int(res[0]), "above": int(res[1]), "sum_var_q16": int(res[2]), "bins": [int(v) for v in res[3:]]}
    return sigma, d


ADAPTIVE_DEFAULTS = {"tolerance": 1.0, "min_samples": 4, "max_samples": 0, "tile_pixels": 1}      # dr_adaptive_defaults


def _adaptive_words(params):
    """a dr_adaptive_params as four words (float, int, int, int)"""
    p = dict(ADAPTIVE_DEFAULTS, **params)
    w = np.zeros(4, np.int32)
    w[:1] = np.array([p["tolerance"]], np.float32).view(np.int32)
    w[1:] = [int(p["min_samples"]), int(p["max_samples"]), int(p["tile_pixels"])]
    return w


def adaptive_select(acc, hist, m2, settings13, divide_by, **params):
    """dr_render_adaptive's selection on the host (device_adaptive.hpp): the accumulator's planes as error() takes them, params = fields of
    dr_adaptive_params -> (flags uint8[gx * gy], tile = block column * gy + row; dict active_tiles, asking_pixels, tiles, pixels, gx, gy)."""
    acc = _arr(acc, np.int32)
    W, H = acc.shape[0], acc.shape[1]
    st, m2, hist = _arr(settings13, np.float32), _arr(m2, np.uint64, (W, H)), _arr(hist, np.int32, (W, H))
    d = _div(st)
    flags, counts, grid, words = np.zeros(max(1, (W // d // 8) * (H // d // 8)), np.uint8), np.zeros(2, np.int64), np.zeros(2, np.int32), _adaptive_words(params)
    _ok(lib().hk_adaptive_select(acc.ctypes.data, _ptr(hist), m2.ctypes.data, W, H, int(divide_by), st.ctypes.data, words.ctypes.data, flags.ctypes.data,
                                 counts.ctypes.data, grid.ctypes.data))
    tiles = int(grid[0]) * int(grid[1])
    return flags[:tiles], {"tiles": tiles, "active_tiles": int(counts[0]), "pixels": 64 * tiles, "asking_pixels": int(counts[1]), "gx": int(grid[0]), "gy": int(grid[1])}


def _order_split(entry, order, region_start, key, regions, with_list):
    """device_split.hpp order_split_plain through hk_sky_split / hk_subset_split: (the entry's count, launch_order int32[tiles], launch_region_start
    int32[17], the dropped tiles int32[tiles] or None)"""
    rs, o, tiles = _arr(region_start, np.int32), _arr(order, np.int32), len(key)
    lo, lrs, dropped = np.zeros(max(1, tiles), np.int32), np.zeros(17, np.int32), np.zeros(max(1, tiles), np.int32) if with_list else None
    n = entry(_ptr(o), rs.ctypes.data, key.ctypes.data, tiles, int(regions), lo.ctypes.data, lrs.ctypes.data, *([dropped.ctypes.data] if with_list else []))
    return n, lo, lrs, dropped


def subset_split(order, region_start, flags, regions):
    """The split by device_adaptive.hpp FlagKeep (hk_subset_split): order int32[tiles] or None (identity), region_start int32[regions + 1 or more], flags
    uint8[tiles] -> (launch_order int32[flagged tiles], launch_region_start int32[17])."""
    n, lo, lrs, _ = _order_split(lib().hk_subset_split, order, region_start, _arr(flags, np.uint8), regions, False)
    return lo[:n], lrs


def adaptive_add(acc, hist, m2, settings13, frames, tiles):
    """dr_render_adaptive's fold on the host (device_adaptive.hpp ad_fold_pixel): frames int32[n, W, H, 3] into acc int32[W, H, 3], m2 uint64[W, H]
    and hist int32[W, H] (+= n) at the pixels of the listed tiles, IN PLACE; the planes must be C-contiguous arrays of exactly these types."""
    assert acc.dtype == np.int32 and m2.dtype == np.uint64 and hist.dtype == np.int32 and acc.flags.c_contiguous and m2.flags.c_contiguous and hist.flags.c_contiguous
    W, H = acc.shape[0], acc.shape[1]
    frames, st, tiles = _arr(frames, np.int32), _arr(settings13, np.float32), _arr(tiles, np.int32)
    assert frames.ndim == 4 and frames.shape[1:] == (W, H, 3) and m2.shape == (W, H) and hist.shape == (W, H)
    _ok(lib().hk_adaptive_add(acc.ctypes.data, hist.ctypes.data, m2.ctypes.data, W, H, st.ctypes.data, frames.ctypes.data, frames.shape[0], _ptr(tiles), len(tiles)))
    return acc, hist, m2


def site_use(hold_order, has_subset):
    """launch_state.hpp site_use -> (hold, sky_split, subset_pair)"""
    u = lib().hk_site_use(int(bool(hold_order)), int(bool(has_subset)))
    return bool(u & 1), bool(u & 2), bool(u & 4)


BUILD_FIELDS = ("count", "occ", "trav_min", "park_min", "unroll", "wide", "coop", "perframe")
PLAN_FIELDS = BUILD_FIELDS + ("blocks", "log_waves", "clear_wave_log")
CFG_FIELDS = ("traversal", "occupancy", "schedule", "num_cus", "coop_tiles_per_wave", "count")
TRACE_PLAN_FIELDS = ("kernel", "traversal", "blocks")


def _cfg(cfg):
    return (C.c_int * 6)(*[int(cfg[k]) for k in CFG_FIELDS])


def _ints(n, call, *args):
    """the n ints an entry writes behind its last argument"""
    out = (C.c_int * n)()
    call(*args, out)
    return tuple(out)


def persistent_plan(cfg, work, coop_steps, per_frame, wave_log_on):
    """launch_plan.hpp plan_persistent: cfg is a dict with CFG_FIELDS -> the plan as a tuple of ints in the order of PLAN_FIELDS (the build's
    eight template arguments first)."""
    return _ints(11, lib().hk_persistent_plan, _cfg(cfg), int(work), int(coop_steps), int(per_frame), int(wave_log_on))


def persistent_can_store_per_frame(cfg):
    return bool(lib().hk_persistent_can_store_per_frame(_cfg(cfg)))


def persistent_builds():
    """The instantiations of render_persistent_kernel (DR_PERSISTENT_BUILDS) as a list of tuples in the order of BUILD_FIELDS."""
    n = lib().hk_persistent_builds(None, 0)
    out = np.zeros((n, 8), np.int32)
    assert lib().hk_persistent_builds(out.ctypes.data, n) == n
    return [tuple(int(v) for v in row) for row in out]


def trace_plan(n, traversal, has_wide, num_cus=256, force=0):
    """launch_plan.hpp plan_trace -> (kernel: 0 one ray per lane / 1 persistent, the traversal really walked, workgroups)"""
    return _ints(3, lib().hk_trace_plan, int(n), int(traversal), int(bool(has_wide)), int(num_cus), int(force))


def radiance_plan(n, traversal, has_wide, num_cus=256, force=0):
    """launch_plan.hpp plan_radiance -> (kernel: 0 one ray per lane / 1 persistent, the traversal really walked, workgroups)"""
    return _ints(3, lib().hk_radiance_plan, int(n), int(traversal), int(bool(has_wide)), int(num_cus), int(force))


def allhits_plan(n, has_wide, num_cus=256, force=0):
    """launch_plan.hpp plan_allhits -> (kernel: 0 one ray per lane / 1 persistent, wide 1 / 0, workgroups)"""
    return _ints(3, lib().hk_allhits_plan, int(n), int(bool(has_wide)), int(num_cus), int(force))


def plan_sky_split(cfg, work, coop_steps, per_frame, wave_log_on):
    """launch_plan.hpp plan_sky_split of persistent_plan's plan for the same arguments: may the launch leave its sky tiles to sky_tiles_kernel"""
    return bool(lib().hk_plan_sky_split(_cfg(cfg), int(work), int(coop_steps), int(per_frame), int(wave_log_on)))


def sky_split(order, region_start, word, regions):
    """The split by device_sky.hpp SkyKeep (hk_sky_split): order int32[tiles] or None (identity), region_start int32[regions + 1 or more], word
    uint32[tiles] -> (launch_order int32[geometry tiles], launch_region_start int32[17], sky_list int32[sky tiles])."""
    n, lo, lrs, sky = _order_split(lib().hk_sky_split, order, region_start, _arr(word, np.uint32), regions, True)
    return lo[:len(word) - n], lrs, sky[:n]


def sky_units(n_sky, batch, chunk):
    """launch_plan.hpp sky_units: the units (sky tile, chunk of frames) of a launch of `batch` frames with n_sky sky tiles; chunk 0 = the whole batch"""
    return int(lib().hk_sky_units(int(n_sky), int(batch), int(chunk)))


def sky_unit(u, batch, chunk):
    """launch_plan.hpp sky_unit: unit u as (position in sky_list, first frame, frames)"""
    return _ints(3, lib().hk_sky_unit, int(u), int(batch), int(chunk))


def plan_regions(tiles, batch_hint, xcd_regions, short_one_queue, tiles_per_wave, num_cus):
    return int(lib().hk_plan_regions(int(tiles), int(batch_hint), int(xcd_regions), int(short_one_queue), int(tiles_per_wave), int(num_cus)))


def plan_split_limit(num_cus, occupancy, split_parts, split_waves):
    return int(lib().hk_plan_split_limit(int(num_cus), int(occupancy), int(split_parts), int(split_waves)))


def cursor_take(cursor, stride, skew=0):
    """launch_plan.hpp cursor_take: (first word of the launch's block of queue cursors, the cursor behind it, the ring is cleared first)"""
    block, nxt, wrap = _ints(3, lib().hk_cursor_take, int(cursor), int(stride), int(skew))
    return block, nxt, bool(wrap)


def cursor_layout():
    """launch_plan.hpp's cursor constants: default stride, largest stride, words of a line, launches a ring lasts at most, words allocated, slots of a block"""
    return dict(zip(("stride", "stride_max", "line_words", "ring_launches", "alloc_words", "slots"), _ints(6, lib().hk_cursor_layout)))


def cursor_ring_blocks(stride, skew=0):
    return int(lib().hk_cursor_ring_blocks(int(stride), int(skew)))


KEY_FIELDS = ("W", "H", "stripe_mod", "stripe_rem", "ncols", "gy", "regions", "scene_gen", "cert_factor", "cert_levels", "camera_entry", "camera_cert")
WORDS_PLANS = ("not wanted", "reuse", "skip: held", "skip: first sight", "compute")


class LaunchState:
    """launch_state.hpp's three states (tile order, camera words, sky split) and the rules on them (hk_order_*, hk_camera_words_*, hk_sky_split_launch).
    A view is (settings13, dict of KEY_FIELDS)."""

    def __init__(self):
        self.h = lib().hk_launch_state_new()

    def __del__(self):
        try:
            lib().hk_launch_state_free(self.h)
        except Exception:
            pass

    @staticmethod
    def _key(view):
        st, k = view
        return _arr(st, np.float32, (13,)), np.array([int(k[f]) for f in KEY_FIELDS], np.int64)

    def read(self):
        """the whole state as a dict: order / words / sky, keys as (tuple of settings13's 13 words, tuple of KEY_FIELDS' values)"""
        w = np.zeros(96, np.int64)
        lib().hk_launch_state_read(self.h, w.ctypes.data)
        w = [int(v) for v in w]
        key = lambda at: (tuple(w[at:at + 13]), tuple(w[at + 13:at + 25]))
        return {"order": {"valid": w[0], "capacity": w[1], "age": w[2], "gen": w[3], "args": tuple(w[4:9]), "key": key(9)},
                "words": {"valid": w[34], "cert_ok": w[35], "entry_ok": w[36], "tiles": w[37], "gen": w[38], "key": key(39), "seen": key(64)},
                "sky": {"valid": w[89], "last": w[90], "words_gen": w[91], "ordered": w[92], "order_gen": w[93], "tiles": w[94], "regions": w[95]}}

    def invalidate(self, order=False, words=False, sky=False):
        lib().hk_launch_state_invalidate(self.h, int(bool(order)) + 2 * int(bool(words)) + 4 * int(bool(sky)))

    def order_begin(self, view, tiles, feedback, follows_camera, hold_order):
        """-> (use_order, record_costs, grow)"""
        st, k = self._key(view)
        u = lib().hk_order_begin(self.h, st.ctypes.data, k.ctypes.data, int(tiles), int(feedback), int(follows_camera), int(hold_order))
        return bool(u & 1), bool(u & 2), bool(u & 4)

    def order_end(self, use, feedback_every):
        return bool(lib().hk_order_end(self.h, int(use[0]) + 2 * int(use[1]) + 4 * int(use[2]), int(feedback_every)))

    def order_pipeline_refresh(self, view, tiles, feedback_every):
        st, k = self._key(view)
        return bool(lib().hk_order_pipeline_refresh(self.h, st.ctypes.data, k.ctypes.data, int(tiles), int(feedback_every)))

    def camera_words_plan(self, view, want_cert, want_entry, wide, tiles, hold_order, batch):
        """-> one of WORDS_PLANS"""
        st, k = self._key(view)
        return WORDS_PLANS[lib().hk_camera_words_plan(self.h, st.ctypes.data, k.ctypes.data, int(want_cert), int(want_entry), int(wide), int(tiles), int(hold_order), int(batch))]

    def camera_words_compute(self, view, tiles, cert_ok, entry_ok):
        st, k = self._key(view)
        lib().hk_camera_words_compute(self.h, st.ctypes.data, k.ctypes.data, int(tiles), int(cert_ok), int(entry_ok))

    def camera_words_readable(self):
        """-> (a certificate can be read back, an entry table can, the launch reads the words)"""
        r = lib().hk_camera_words_readable(self.h)
        return bool(r & 1), bool(r & 2), bool(r & 4)

    def sky_split_launch(self, split, use_order, tiles, regions, room=True):
        """-> the stored split served the launch"""
        return bool(lib().hk_sky_split_launch(self.h, int(split), int(use_order), int(tiles), int(regions), int(room)))


TICKET_PLACES = ("held", "slot", "parked", "finished", "never")
GROUP_PLAN_FIELDS = ("start_behind", "host_wait_slot", "stream_wait_slot", "slot_last", "wait_barrier", "alone", "wait_streams")


class PipelineBook:
    """pipeline_state.hpp's ticket book with an integer for a frame's image, the slots' images and the group between group_begin and group_commit
    (hk_pipeline_*).  A view is an integer (hk_pipeline.hpp)."""
    PARKED_MAX = property(lambda self: lib().hk_pipeline_parked_max())

    def __init__(self):
        self.h = lib().hk_pipeline_new()

    def __del__(self):
        try:
            lib().hk_pipeline_free(self.h)
        except Exception:
            pass

    def locate(self, ticket):
        """-> (one of TICKET_PLACES, slot, frame, waited for, presented)"""
        out = (C.c_int * 5)()
        lib().hk_pipeline_locate(self.h, ticket, out)
        return TICKET_PLACES[out[0]], out[1], out[2], bool(out[3]), bool(out[4])

    def submit_closes(self, view, seed):
        return bool(lib().hk_pipeline_submit_closes(self.h, view, seed))

    def owed_after(self, launches):
        return lib().hk_pipeline_owed_after(self.h, launches)

    def submit_overfills(self, closes):
        return bool(lib().hk_pipeline_submit_overfills(self.h, int(closes)))

    def hold(self, view, seed, div):
        return lib().hk_pipeline_hold(self.h, view, seed, div)

    def group_full(self, room):
        return bool(lib().hk_pipeline_group_full(self.h, room))

    def flush_size(self, room):
        return lib().hk_pipeline_flush_size(self.h, room)

    def drop_held(self):
        lib().hk_pipeline_drop_held(self.h)

    def group_begin(self, n):
        """-> (slot, stream, first ticket, seed stride, tuple of the frames to park)"""
        out = np.zeros(5 + 16, np.int64)
        lib().hk_pipeline_group_begin(self.h, n, out.ctypes.data)
        return int(out[0]), int(out[1]), int(out[2]) % 2 ** 64, int(out[3]) % 2 ** 64, tuple(int(v) for v in out[5:5 + int(out[4])])

    def group_plan(self, refresh, cursor_wraps):
        """-> dict of GROUP_PLAN_FIELDS"""
        out = (C.c_int * 7)()
        lib().hk_pipeline_group_plan(self.h, int(refresh), int(cursor_wraps), out)
        return dict(zip(GROUP_PLAN_FIELDS, (int(v) for v in out)))

    def group_take_slot(self):
        lib().hk_pipeline_group_take_slot(self.h)

    def group_commit(self, tokens):
        t = np.array(list(tokens), np.int64)
        lib().hk_pipeline_group_commit(self.h, t.ctypes.data)

    def mark_waited(self, ticket):
        return bool(lib().hk_pipeline_mark_waited(self.h, ticket))

    def image(self, ticket):
        return lib().hk_pipeline_image(self.h, ticket)

    def all_drained(self):
        lib().hk_pipeline_all_drained(self.h)

    def join(self):
        """join_plan and joined -> (tuple of the (slot, frame) whose adds `stream` waits for, mask of the streams whose newest launch)"""
        out = (C.c_int * 12)()
        lib().hk_pipeline_join(self.h, out)
        n = out[0]
        return tuple((out[1 + 2 * k], out[2 + 2 * k]) for k in range(n)), out[1 + 2 * n]

    def restart_numbering(self, streams):
        lib().hk_pipeline_restart_numbering(self.h, streams)

    def dump(self):
        """the whole book as a tuple of ints (hk_pipeline_dump lists the words)"""
        n = lib().hk_pipeline_dump(self.h, None, 0)
        out = np.zeros(n, np.int64)
        lib().hk_pipeline_dump(self.h, out.ctypes.data, n)
        return tuple(int(v) % 2 ** 64 for v in out)
