"""dogeray_amd -- MI355X-native render path for DOGERAY scenes.

Thin ctypes binding of libdogeray_amd.so (C ABI in include/dogeray_amd.h).  All rendering
happens in the HIP library; there is no Python or CPU fallback: if the shared library is
missing or no GPU is present the calls below raise.

The Python surface mirrors the reference's host flow (kernel.cu main(), K:2021-2557):
    Scene.load(path, texture_dir)   ~ getnum + getppm* + read            (K:2055-2071)
    scene.build_bvh()               ~ build_bvh                          (K:2091)
    Context(device).upload(scene)   ~ what CudaStarter re-uploads per frame (K:2618-2629)
    ctx.render_frame(settings13, ...)  ~ CudaStarter(outputr, ..., divisor) (K:2562)
    ProgressiveRenderer             ~ the present loop's preview ladder + accumulation (K:2154-2224)
"""
import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("DOGERAY_AMD_LIB") or os.path.join(_HERE, "libdogeray_amd.so")      # the override serves kernel experiments

TRAVERSAL_THREADED = 0
TRAVERSAL_ORDERED = 1
TRAVERSAL_WIDE = 2          # the default: 4-way tree over the reference's leaves
KERNEL_TILE = 0
KERNEL_PERSISTENT = 1
MAX_REGIONS = 8             # tile queues of the persistent kernel (csrc/launch_plan.hpp)
ERR_INVALID, ERR_IO, ERR_PARSE, ERR_SCENE, ERR_DEVICE, ERR_NOMEM = -1, -2, -3, -4, -5, -6      # enum dr_status


class DogerayError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("dogeray_amd error %d: %s" % (code, msg))
        self.code = code


class DrObject(C.Structure):
    _fields_ = [("type", C.c_int32), ("pos", C.c_float * 3), ("rot", C.c_float * 3), ("norm", C.c_float * 3),
                ("n1", C.c_float * 3), ("n2", C.c_float * 3), ("n3", C.c_float * 3), ("t1", C.c_float * 3),
                ("t2", C.c_float * 3), ("t3", C.c_float * 3), ("smooth", C.c_int32), ("tex", C.c_int32),
                ("mat", C.c_int32), ("dim", C.c_float * 3), ("col", C.c_float * 3), ("texnum", C.c_int32),
                ("rtexnum", C.c_int32), ("addional", C.c_float * 3)]


OBJECT_DTYPE = np.dtype([("type", "<i4"), ("pos", "<f4", 3), ("rot", "<f4", 3), ("norm", "<f4", 3),
                         ("n1", "<f4", 3), ("n2", "<f4", 3), ("n3", "<f4", 3), ("t1", "<f4", 3), ("t2", "<f4", 3),
                         ("t3", "<f4", 3), ("smooth", "<i4"), ("tex", "<i4"), ("mat", "<i4"), ("dim", "<f4", 3),
                         ("col", "<f4", 3), ("texnum", "<i4"), ("rtexnum", "<i4"), ("addional", "<f4", 3)])
BVH_DTYPE = np.dtype([("active", "<i4"), ("children", "<i4", 2), ("count", "<i4"), ("hit_node", "<i4"),
                      ("miss_node", "<i4"), ("under", "<i4"), ("min", "<f4", 3), ("max", "<f4", 3), ("end", "<i4")])


class DrSettings(C.Structure):
    _fields_ = [("campos", C.c_float * 3), ("look", C.c_float * 3), ("aperture", C.c_float),
                ("focus_dist", C.c_float), ("fov", C.c_int32), ("max_depth", C.c_int32), ("spp", C.c_int32),
                ("background", C.c_float), ("backtex", C.c_int32), ("width", C.c_int32), ("height", C.c_int32)]


class DrStats(C.Structure):
    _fields_ = [("frames", C.c_uint64), ("launches", C.c_uint64), ("samples", C.c_uint64), ("rays", C.c_uint64), ("node_visits", C.c_uint64),
                ("prim_tests", C.c_uint64), ("shades", C.c_uint64), ("texels", C.c_uint64), ("kernel_ms", C.c_double),
                ("trav_slots", C.c_uint64), ("ray_slots", C.c_uint64), ("diag", C.c_uint64 * 8)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["diag"] = list(self.diag)
        return d


class DrAovBuffers(C.Structure):
    """struct dr_aov_buffers: one pointer per first-hit channel (NULL: not computed)."""
    _fields_ = [("t", C.c_void_p), ("distance", C.c_void_p), ("depth", C.c_void_p), ("object", C.c_void_p), ("material", C.c_void_p),
                ("normal", C.c_void_p), ("uv", C.c_void_p), ("albedo", C.c_void_p), ("dir", C.c_void_p)]


# the channels of Context.render_aov: name -> (dtype, components per pixel)
AOV_CHANNELS = {"t": (np.float32, 1), "distance": (np.float32, 1), "depth": (np.float32, 1), "object": (np.int32, 1), "material": (np.int32, 1),
                "normal": (np.float32, 3), "uv": (np.float32, 2), "albedo": (np.float32, 3), "dir": (np.float32, 3)}
ALL = tuple(AOV_CHANNELS)


class DrAovLensBuffers(C.Structure):
    """struct dr_aov_lens_buffers: one pointer per lens-averaged channel (NULL: not computed)."""
    _fields_ = [("coverage", C.c_void_p), ("depth", C.c_void_p), ("distance", C.c_void_p), ("material", C.c_void_p), ("normal", C.c_void_p),
                ("albedo", C.c_void_p)]


# the channels of Context.render_aov_lens: name -> (dtype, components per pixel)
AOV_LENS_CHANNELS = {"coverage": (np.float32, 1), "depth": (np.float32, 1), "distance": (np.float32, 1), "material": (np.int32, 1),
                     "normal": (np.float32, 3), "albedo": (np.float32, 3)}
GUIDE_SEED = 0x67756964656C656E      # DR_GUIDE_SEED: the frame seed of the guides option "guide_frames" traces


class DrRayBuffers(C.Structure):
    """struct dr_ray_buffers (include/dogeray_amd.h dr_trace_rays): origin, dir (3 floats per ray), tmax (one, or NULL)."""
    _fields_ = [("origin", C.c_void_p), ("dir", C.c_void_p), ("tmax", C.c_void_p)]


class DrHitBuffers(C.Structure):
    """struct dr_hit_buffers: one pointer per channel of dr_trace_rays (NULL: not computed)."""
    _fields_ = [("t", C.c_void_p), ("object", C.c_void_p), ("material", C.c_void_p), ("distance", C.c_void_p), ("normal", C.c_void_p),
                ("uv", C.c_void_p), ("albedo", C.c_void_p), ("occluded", C.c_void_p)]


# the channels of Context.trace: name -> (dtype, components per ray); "occluded" is what any_hit=True returns
TRACE_CHANNELS = {"t": (np.float32, 1), "object": (np.int32, 1), "material": (np.int32, 1), "distance": (np.float32, 1), "normal": (np.float32, 3),
                  "uv": (np.float32, 2), "albedo": (np.float32, 3)}
TRACE_CLOSEST, TRACE_ANY = 0, 1


class DrRadianceParams(C.Structure):
    """struct dr_radiance_params (include/dogeray_amd.h dr_trace_radiance)."""
    _fields_ = [("spp", C.c_int), ("max_depth", C.c_int), ("background", C.c_float), ("backtex", C.c_int), ("seed", C.c_uint64)]


class DrRadianceRays(C.Structure):
    """struct dr_radiance_rays: origin, dir (3 floats per ray), seed (uint64 per ray, or NULL), skip (int32 per ray, or NULL)."""
    _fields_ = [("origin", C.c_void_p), ("dir", C.c_void_p), ("seed", C.c_void_p), ("skip", C.c_void_p)]


class DrRadianceOut(C.Structure):
    """struct dr_radiance_out: radiance (3 floats per ray), bounces (int32 per ray); NULL: not computed."""
    _fields_ = [("radiance", C.c_void_p), ("bounces", C.c_void_p)]


# the channels of Context.radiance: name -> (dtype, components per ray)
RADIANCE_CHANNELS = {"radiance": (np.float32, 3), "bounces": (np.int32, 1)}


class DrPointBuffers(C.Structure):
    """struct dr_point_buffers (include/dogeray_amd.h dr_query_nearest): point (3 floats per query), rmax (one, or NULL)."""
    _fields_ = [("point", C.c_void_p), ("rmax", C.c_void_p)]


class DrNearestBuffers(C.Structure):
    """struct dr_nearest_buffers: one pointer per channel of dr_query_nearest (NULL: not computed)."""
    _fields_ = [("distance", C.c_void_p), ("d2", C.c_void_p), ("object", C.c_void_p), ("material", C.c_void_p), ("point", C.c_void_p),
                ("uv", C.c_void_p)]


# the channels of Context.nearest: name -> (dtype, components per query)
NEAREST_CHANNELS = {"distance": (np.float32, 1), "d2": (np.float32, 1), "object": (np.int32, 1), "material": (np.int32, 1), "point": (np.float32, 3),
                    "uv": (np.float32, 2)}


class DrAllHitsParams(C.Structure):
    """struct dr_allhits_params (include/dogeray_amd.h dr_trace_all_hits)."""
    _fields_ = [("max_hits", C.c_int), ("kind_mask", C.c_int)]


class DrAllHitsBuffers(C.Structure):
    """struct dr_allhits_buffers: one pointer per channel of dr_trace_all_hits (NULL: not computed)."""
    _fields_ = [("count", C.c_void_p), ("t", C.c_void_p), ("object", C.c_void_p), ("material", C.c_void_p), ("distance", C.c_void_p),
                ("normal", C.c_void_p), ("uv", C.c_void_p), ("albedo", C.c_void_p)]


# the channels of Context.trace_all: name -> (dtype, components per listed hit; 0: one value per ray)
ALLHITS_CHANNELS = {"count": (np.int32, 0), "t": (np.float32, 1), "object": (np.int32, 1), "material": (np.int32, 1), "distance": (np.float32, 1),
                    "normal": (np.float32, 3), "uv": (np.float32, 2), "albedo": (np.float32, 3)}
ALLHITS_MAX = 8                                   # DR_ALLHITS_MAX
ALLHITS_KINDS = {"triangle": 1, "sphere": 2}      # DR_ALLHITS_TRIANGLES, DR_ALLHITS_SPHERES
# Context.contains: three fixed directions, none along an axis, no two orthogonal (pairwise dot products 11, -1, 5)
CONTAINS_DIRECTIONS = ((1.0, 2.0, 3.0), (3.0, 1.0, 2.0), (2.0, -3.0, 1.0))


class DrDenoiseParams(C.Structure):
    """struct dr_denoise_params (include/dogeray_amd.h dr_accum_denoise)."""
    _fields_ = [("iterations", C.c_int), ("sigma_luminance", C.c_float), ("normal_power_log2", C.c_int), ("sigma_depth", C.c_float),
                ("demodulate", C.c_int), ("material_stop", C.c_int)]


class DrUpscaleParams(C.Structure):
    """struct dr_upscale_params (include/dogeray_amd.h dr_accum_upscale)."""
    _fields_ = [("mode", C.c_int), ("normal_power_log2", C.c_int), ("sigma_depth", C.c_float), ("demodulate", C.c_int), ("material_stop", C.c_int)]


UPSCALE_BLOCK, UPSCALE_GUIDED = 0, 1


class DrReprojectParams(C.Structure):
    """struct dr_reproject_params (include/dogeray_amd.h dr_accum_reproject)."""
    _fields_ = [("max_history", C.c_int), ("normal_cos", C.c_float), ("plane_tolerance", C.c_float), ("material_mask", C.c_uint32), ("sky", C.c_int)]


class DrReprojectResult(C.Structure):
    """struct dr_reproject_result: grid pixels per class; pixels = valid + masked + offscreen + rejected."""
    _fields_ = [("pixels", C.c_int64), ("valid", C.c_int64), ("masked", C.c_int64), ("offscreen", C.c_int64), ("rejected", C.c_int64)]


class DrErrorResult(C.Structure):
    """struct dr_error_result (include/dogeray_amd.h dr_accum_error): counts over the pixel grid and the fixed-point sum of the variances."""
    _fields_ = [("pixels", C.c_int64), ("estimated", C.c_int64), ("above", C.c_int64), ("sum_var_q16", C.c_uint64), ("bins", C.c_int64 * 16)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "bins"}
        d["bins"] = [int(v) for v in self.bins]
        return d


class DrAdaptiveParams(C.Structure):
    """struct dr_adaptive_params (include/dogeray_amd.h dr_render_adaptive)."""
    _fields_ = [("tolerance", C.c_float), ("min_samples", C.c_int), ("max_samples", C.c_int), ("tile_pixels", C.c_int)]


class DrAdaptiveResult(C.Structure):
    """struct dr_adaptive_result: the tiles and pixels of one pass; samples_added = active_tiles * 64 * nframes."""
    _fields_ = [("tiles", C.c_int64), ("active_tiles", C.c_int64), ("pixels", C.c_int64), ("asking_pixels", C.c_int64), ("samples_added", C.c_int64)]


# every symbol include/dogeray_amd.h declares: (name, restype, argtypes)
_VP = C.c_void_p
_API = [
    ("dr_last_error", C.c_char_p, []),
    ("dr_abi_version", C.c_int, []),
    ("dr_scene_load", C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(_VP)]),
    ("dr_scene_free", None, [_VP]),
    ("dr_scene_create_from_arrays", C.c_int, [_VP, C.c_int, C.POINTER(DrSettings), _VP, C.c_int, C.POINTER(_VP)]),
    ("dr_scene_add_texture", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_char_p]),
    ("dr_scene_num_objects", C.c_int, [_VP]),
    ("dr_scene_get_objects", C.c_int, [_VP, _VP]),
    ("dr_scene_get_settings", C.c_int, [_VP, C.POINTER(DrSettings)]),
    ("dr_scene_set_settings", C.c_int, [_VP, C.POINTER(DrSettings)]),
    ("dr_scene_num_textures", C.c_int, [_VP]),
    ("dr_scene_texture_info", C.c_int, [_VP, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("dr_scene_texture_data", C.c_int, [_VP, C.c_int, _VP]),
    ("dr_scene_build_bvh", C.c_int, [_VP, C.c_int]),
    ("dr_scene_bvh_size", C.c_int, [_VP]),
    ("dr_scene_bvh_used", C.c_int, [_VP]),
    ("dr_scene_get_bvh", C.c_int, [_VP, _VP]),
    ("dr_scene_save_binary", C.c_int, [_VP, C.c_char_p]),
    ("dr_scene_load_binary", C.c_int, [C.c_char_p, C.POINTER(_VP)]),
    ("dr_device_count", C.c_int, []),
    ("dr_context_create", C.c_int, [C.c_int, C.POINTER(_VP)]),
    ("dr_context_destroy", None, [_VP]),
    ("dr_context_upload_scene", C.c_int, [_VP, _VP]),
    ("dr_context_set_stripe", C.c_int, [_VP, C.c_int, C.c_int]),
    ("dr_context_set_traversal", C.c_int, [_VP, C.c_int]),
    ("dr_context_set_option", C.c_int, [_VP, C.c_char_p, C.c_int]),
    ("dr_context_get_option", C.c_int, [_VP, C.c_char_p, C.POINTER(C.c_int)]),
    ("dr_render_frame", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_float, C.c_uint64, _VP]),
    ("dr_accum_reset", C.c_int, [_VP, C.c_int, C.c_int]),
    ("dr_render_accumulate", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_int]),
    ("dr_accum_read", C.c_int, [_VP, _VP]),
    ("dr_accum_present", C.c_int, [_VP, C.c_int, _VP]),
    ("dr_accum_device_ptr", C.c_int, [_VP, C.POINTER(_VP), C.POINTER(C.c_uint64)]),
    ("dr_accum_history_read", C.c_int, [_VP, _VP]),
    ("dr_accum_history_device_ptr", C.c_int, [_VP, C.POINTER(_VP), C.POINTER(C.c_uint64)]),
    ("dr_accum_moments_read", C.c_int, [_VP, _VP]),
    ("dr_accum_moments_device_ptr", C.c_int, [_VP, C.POINTER(_VP), C.POINTER(C.c_uint64)]),
    ("dr_accum_error", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.c_float, _VP, C.POINTER(DrErrorResult), C.c_int]),
    ("dr_adaptive_defaults", C.c_int, [C.POINTER(DrAdaptiveParams)]),
    ("dr_render_adaptive", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(DrAdaptiveParams),
                                     C.POINTER(DrAdaptiveResult)]),
    ("dr_reproject_defaults", C.c_int, [C.POINTER(DrReprojectParams)]),
    ("dr_accum_reproject", C.c_int, [_VP, _VP, _VP, C.c_int, C.c_int, C.c_int, C.POINTER(DrReprojectParams), C.POINTER(DrReprojectResult)]),
    ("dr_render_accumulate_async", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_int]),
    ("dr_context_synchronize", C.c_int, [_VP]),
    ("dr_pipeline_submit", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]),
    ("dr_pipeline_wait", C.c_int, [_VP, C.c_uint64, _VP]),
    ("dr_pipeline_image", C.c_int, [_VP, C.c_uint64, C.POINTER(_VP)]),
    ("dr_render_accumulate_pipelined", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_int]),
    ("dr_context_stream", C.c_int, [_VP, C.POINTER(_VP)]),
    ("dr_accum_pack_stripe", C.c_int, [_VP, C.c_int, C.POINTER(_VP), C.POINTER(C.c_uint64)]),
    ("dr_accum_unpack_stripes", C.c_int, [_VP, _VP, C.c_uint64, C.c_int, C.c_int, _VP]),
    ("dr_accum_reserve_pack", C.c_int, [_VP, C.c_int]),
    ("dr_render_aov", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(DrAovBuffers), C.c_int]),
    ("dr_render_aov_lens", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int,
                                     C.POINTER(DrAovLensBuffers), C.c_int]),
    ("dr_trace_rays", C.c_int, [_VP, C.c_int, C.c_int64, C.POINTER(DrRayBuffers), C.POINTER(DrHitBuffers), C.c_int]),
    ("dr_radiance_defaults", C.c_int, [C.POINTER(DrRadianceParams)]),
    ("dr_trace_radiance", C.c_int, [_VP, C.c_int64, C.POINTER(DrRadianceRays), C.POINTER(DrRadianceParams), C.POINTER(DrRadianceOut), C.c_int]),
    ("dr_query_nearest", C.c_int, [_VP, C.c_int64, C.POINTER(DrPointBuffers), C.POINTER(DrNearestBuffers), C.c_int]),
    ("dr_allhits_defaults", C.c_int, [C.POINTER(DrAllHitsParams)]),
    ("dr_trace_all_hits", C.c_int, [_VP, C.c_int64, C.POINTER(DrRayBuffers), C.POINTER(DrAllHitsParams), C.POINTER(DrAllHitsBuffers), C.c_int]),
    ("dr_denoise_defaults", C.c_int, [C.POINTER(DrDenoiseParams)]),
    ("dr_accum_denoise", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.POINTER(DrDenoiseParams), _VP, _VP, C.c_int]),
    ("dr_upscale_defaults", C.c_int, [C.POINTER(DrUpscaleParams)]),
    ("dr_accum_upscale", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_int, C.POINTER(DrUpscaleParams), C.POINTER(DrDenoiseParams), _VP, _VP, C.c_int]),
    ("dr_group_create", C.c_int, [C.c_int, _VP, C.POINTER(_VP)]),
    ("dr_group_destroy", None, [_VP]),
    ("dr_group_size", C.c_int, [_VP]),
    ("dr_group_uses_rccl", C.c_int, [_VP]),
    ("dr_group_rccl_ranks", C.c_int, [_VP]),
    ("dr_group_context", _VP, [_VP, C.c_int]),
    ("dr_group_upload_scene", C.c_int, [_VP, _VP]),
    ("dr_group_accum_reset", C.c_int, [_VP, C.c_int, C.c_int]),
    ("dr_group_render_accumulate", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_int, C.c_int]),
    ("dr_stats_enable_counters", C.c_int, [_VP, C.c_int]),
    ("dr_stats_reset", C.c_int, [_VP]),
    ("dr_stats_get", C.c_int, [_VP, C.POINTER(DrStats)]),
    ("dr_context_probe_trace", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("dr_context_probe_rays", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_float, C.c_uint64, _VP, _VP, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("dr_stats_phase_counts", C.c_int, [_VP, C.POINTER(C.c_ulonglong), C.c_int]),
    ("dr_stats_cert_mask", C.c_int, [_VP, _VP, C.c_int, C.POINTER(C.c_int)]),
    ("dr_stats_cert_levels", C.c_int, [_VP, _VP, C.c_int, C.POINTER(C.c_int)]),
    ("dr_stats_camera_entry", C.c_int, [_VP, _VP, C.c_int, C.POINTER(C.c_int)]),
    ("dr_stats_sky_tiles", C.c_int, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("dr_stats_adaptive_tiles", C.c_int, [_VP, _VP, C.c_int, C.POINTER(C.c_int)]),
    ("dr_stats_wave_log", C.c_int, [_VP, C.POINTER(C.c_ulonglong), C.c_int, C.POINTER(C.c_int)]),
    ("dr_stats_pixel_cost", C.c_int, [_VP, C.POINTER(C.c_uint), C.c_size_t, C.POINTER(C.c_size_t)]),
    ("dr_context_probe_gather", C.c_int, [_VP, C.c_uint32, C.c_int, C.POINTER(C.c_double)]),
    ("dr_context_probe_frame_add", C.c_int, [_VP, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("dr_kat_rng", C.c_int, [_VP, C.c_uint64, C.c_int, _VP]),
    ("dr_kat_aabb", C.c_int, [_VP, C.c_int] + [_VP] * 6),
    ("dr_kat_tri", C.c_int, [_VP, C.c_int] + [_VP] * 6),
    ("dr_kat_node_planes", C.c_int, [_VP, C.c_int] + [_VP] * 5),
    ("dr_kat_sphere", C.c_int, [_VP, C.c_int] + [_VP] * 5),
    ("dr_kat_optics", C.c_int, [_VP, C.c_int] + [_VP] * 6),
    ("dr_kat_hit", C.c_int, [_VP, C.c_int] + [_VP] * 5),
    ("dr_kat_normal", C.c_int, [_VP, C.c_int] + [_VP] * 6),
    ("dr_kat_trace", C.c_int, [_VP, C.c_int, C.c_int] + [_VP] * 4),
    ("dr_kat_sample", C.c_int, [_VP, C.c_int] + [_VP] * 7),
    ("dr_kat_outside", C.c_int, [_VP, C.c_int, _VP, _VP]),
    ("dr_kat_tex", C.c_int, [_VP, C.c_int] + [_VP] * 4),
    ("dr_kat_bounce", C.c_int, [_VP, C.c_int] + [_VP] * 12),
    ("dr_kat_miss", C.c_int, [_VP, C.c_int, _VP, _VP, C.c_int, C.c_float, _VP]),
    ("dr_kat_camera", C.c_int, [_VP, _VP, C.c_int, C.c_int, C.c_uint64, C.c_uint32, C.c_int] + [_VP] * 6),
    ("dr_kat_store", C.c_int, [_VP, C.c_int, _VP, C.c_int, _VP]),
    ("dr_kat_store_merged", C.c_int, [_VP, C.c_int, C.c_int] + [_VP] * 5 + [C.c_int] * 3 + [_VP] * 3),
    ("dr_stats_tile_order", C.c_int, [_VP, _VP, C.c_size_t, C.POINTER(C.c_size_t), _VP, _VP]),
    ("dr_kat_tile_feedback", C.c_int, [_VP] + [C.c_int] * 5 + [_VP] * 4),
    ("dr_kat_order_split", C.c_int, [_VP] + [C.c_int] * 3 + [_VP] * 7),
]
API_SYMBOLS = [a[0] for a in _API]

_lib = None


def lib():
    """The loaded libdogeray_amd.so.  Raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError("libdogeray_amd.so is missing: run `python -m dogeray_amd.build` "
                              "(or __graft_entry__.build()); dogeray_amd has no fallback path")
        # One process must hold ONE HIP runtime.  PyTorch-ROCm ships its own libamdhip64; if this
        # library pulled in /opt/rocm's copy first, torch's later initialisation finds "no HIP GPUs".
        # Importing torch first (when it is installed) makes both resolve to the same runtime.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(_LIB_PATH)
        for name, res, args in _API:
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise DogerayError(rc, lib().dr_last_error().decode(errors="replace"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- known-answer hooks (dr_kat_*, and their host mirrors tools/host_kernel.py hk_kat_*): n items in, n items out.
# hook -> (inputs: (name, dtype, shape tail) each, an item's array [n] + tail; outputs: (dtype, shape) each, "n" standing for n, in the order
# the wrapper returns them).  Where a hook returns both forms of a step the output has a leading axis of 2.
_U32, _I32, _U64, _F32 = np.uint32, np.int32, np.uint64, np.float32
KAT_HOOKS = {
    "rng": ((), ((np.float64, ("n",)),)),
    "aabb": ((("o", _F32, (3,)), ("d", _F32, (3,)), ("mn", _F32, (3,)), ("mx", _F32, (3,))), ((_I32, ("n",)), (_F32, ("n",)))),
    "tri": ((("o", _F32, (3,)), ("d", _F32, (3,)), ("v0", _F32, (3,)), ("v1", _F32, (3,)), ("v2", _F32, (3,))), ((_F32, ("n",)),)),
    "node_planes": ((("w", _U32, ()), ("a", _F32, ()), ("b", _F32, ())), ((_F32, ("n", 4)), (_F32, ("n", 4)))),
    "sphere": ((("o", _F32, (3,)), ("d", _F32, (3,)), ("c", _F32, (3,)), ("r", _F32, ())), ((_F32, ("n",)),)),
    "optics": ((("v", _F32, (3,)), ("nrm", _F32, (3,)), ("eta", _F32, ())), ((_F32, ("n", 3)), (_F32, ("n", 3)), (_F32, ("n",)))),
    "normal": ((("obj_index", _I32, ()), ("o", _F32, (3,)), ("d", _F32, (3,)), ("t", _F32, ())), ((_F32, ("n", 3)), (_F32, ("n", 3)))),
    "hit": ((("o", _F32, (3,)), ("d", _F32, (3,))), ((_F32, ("n",)), (_I32, ("n",)), (_I32, ("n",)))),
    "trace": ((("o", _F32, (3,)), ("d", _F32, (3,))), ((_F32, ("n",)), (_I32, ("n",)))),
    "sample": ((("seed", _U64, ()), ("warm", _I32, ()), ("kind", _I32, ())), ((_F32, (2, "n", 3)), (_U32, (2, "n", 2)))),
    "outside": ((("d2", _F32, ()),), ((_I32, ("n",)),)),
    "tex": ((("tex", _I32, ()), ("u", _F32, ()), ("v", _F32, ())), ((_U32, ("n",)),)),
    "bounce": ((("obj_index", _I32, ()), ("o", _F32, (3,)), ("d", _F32, (3,)), ("t", _F32, ()), ("atten", _F32, (3,)), ("seed", _U64, ()), ("warm", _I32, ())),
               ((_I32, (2, "n")), (_F32, (2, "n", 3)), (_F32, (2, "n", 3)), (_F32, (2, "n", 3)), (_U32, (2, "n", 2)))),
    "miss": ((("d", _F32, (3,)), ("atten", _F32, (3,))), ((_F32, ("n", 3)),)),
    "camera": ((("x", _I32, ()), ("y", _I32, ()), ("sample", _I32, ())), ((_F32, (2, "n", 3)), (_F32, (2, "n", 3)), (_U32, (2, "n", 2)))),
    "store": ((("color", _F32, (3,)),), ((_I32, ("n", 3)),)),
    "tile_feedback": ((("pixel_cost", _U32, (64,)),), ((_U32, ("n",)), (_I32, ("n",)), (_I32, (2 * MAX_REGIONS + 1,)))),
    "order_split": ((("order", _I32, ()), ("region_start", _I32, ()), ("key", _U32, ())),
                    ((_I32, ("n",)), (_I32, (2 * MAX_REGIONS + 1,)), (_I32, ("n",)), (_U32, (2,)))),
}


def kat_marshal(hook, arrays, call, n=None):
    """The marshalling of a known-answer hook (KAT_HOOKS[hook]): converts `arrays` to the inputs' dtypes, takes n from the first one, raises
    ValueError unless every input is [n] + its tail (leading dimension n, n * prod(tail) elements), allocates the outputs zeroed and calls
    call(n, input pointers, output arrays), which makes the library call and raises on its status.  Returns the outputs as a tuple.  A hook
    that has its own rule for the count (kat_rng, kat_tile_feedback, kat_order_split) passes n: the inputs are then only converted, and the outputs hold
    max(n, 0) items.  Everything before `call` touches no library."""
    ins_spec, outs_spec = KAT_HOOKS[hook]
    assert len(arrays) == len(ins_spec)
    ins = [np.ascontiguousarray(a, dtype=dt) for a, (_, dt, _) in zip(arrays, ins_spec)]
    if n is None:
        n = ins[0].shape[0]
        for a, (name, _, tail) in zip(ins, ins_spec):
            if a.shape[0] != n or a.size != n * int(np.prod(tail, dtype=np.int64)):
                raise ValueError("kat_%s: %s must be [%s]" % (hook, name, ", ".join(["n"] + [str(k) for k in tail])))
    outs = tuple(np.zeros(tuple(max(n, 0) if k == "n" else k for k in shape), dtype=dt) for dt, shape in outs_spec)
    call(n, [_p(a) for a in ins], outs)
    return outs


def device_count():
    return lib().dr_device_count()


def pixel_grid(settings13, W, H):
    """(width, height) of the pixel grid dr_render_frame renders: (W / div / 8) * 8 x (H / div / 8) * 8, div = settings13[11]."""
    div = float(np.float32(settings13[11]))
    div = int(div) if np.isfinite(div) else 0
    if div < 1:
        return 0, 0
    return W // div // 8 * 8, H // div // 8 * 8


def write_pfm(path, img):
    """Portable float map: float32[h, w] ("Pf") or float32[h, w, 3] ("PF"), little-endian; row 0 of the array is the top row of the
    image (the file stores the bottom row first)."""
    a = np.asarray(img, dtype=np.float32)
    if a.ndim == 3 and a.shape[2] == 1:
        a = a[:, :, 0]
    if not (a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3)):
        raise ValueError("write_pfm: need [h, w] or [h, w, 3], got %s" % (a.shape,))
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n-1.0\n" % (b"PF" if a.ndim == 3 else b"Pf", a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a[::-1], dtype="<f4").tobytes())
    return path


def read_pfm(path):
    """The array write_pfm wrote (either byte order on input; float32, row 0 = top row)."""
    with open(path, "rb") as f:
        data = f.read()
    fields, pos = [], 0
    while len(fields) < 4:                 # magic, width, height, scale: whitespace-separated, one whitespace byte after the scale
        while data[pos:pos + 1].isspace():
            pos += 1
        end = pos
        while not data[end:end + 1].isspace():
            end += 1
        fields.append(data[pos:end])
        pos = end
    pos += 1
    magic, w, h, scale = fields[0], int(fields[1]), int(fields[2]), float(fields[3])
    if magic not in (b"PF", b"Pf"):
        raise ValueError("%s is not a PFM file" % path)
    ch = 3 if magic == b"PF" else 1
    a = np.frombuffer(data, dtype="<f4" if scale < 0 else ">f4", count=w * h * ch, offset=pos).astype(np.float32)
    a = a.reshape((h, w, 3) if ch == 3 else (h, w))
    return np.ascontiguousarray(a[::-1])


def _params(struct, defaults_fn, what, **fields):
    """A parameter struct: the library's defaults (defaults_fn) with the given fields replaced."""
    p = struct()
    _check(getattr(lib(), defaults_fn)(C.byref(p)))
    for k, v in fields.items():
        if k not in dict(struct._fields_):
            raise TypeError("unknown %s parameter %r (known: %s)" % (what, k, ", ".join(f[0] for f in struct._fields_)))
        setattr(p, k, v)
    return p


def denoise_params(**params):
    """A DrDenoiseParams: the library's defaults (dr_denoise_defaults) with the given fields replaced."""
    return _params(DrDenoiseParams, "dr_denoise_defaults", "denoise", **params)


def upscale_params(**params):
    """A DrUpscaleParams: the library's defaults (dr_upscale_defaults) with the given fields replaced."""
    return _params(DrUpscaleParams, "dr_upscale_defaults", "upscale", **params)


def reproject_params(**params):
    """A DrReprojectParams: the library's defaults (dr_reproject_defaults) with the given fields replaced."""
    return _params(DrReprojectParams, "dr_reproject_defaults", "reproject", **params)


def adaptive_params(**params):
    """A DrAdaptiveParams: the library's defaults (dr_adaptive_defaults) with the given fields replaced."""
    return _params(DrAdaptiveParams, "dr_adaptive_defaults", "adaptive", **params)


def _out_array(shape, dtype, dev=None):
    """An output of this shape and numpy dtype -- a numpy array, or on dev a torch tensor -- and its address."""
    if dev is None:
        a = np.empty(shape, dtype=dtype)
        return a, a.ctypes.data
    import torch
    a = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=dev)
    return a, a.data_ptr()


def pack_settings13(s, divisor, spp=None, depth=None):
    """float settings[13] exactly as CudaStarter packs it (K:2581)."""
    return np.array([s.campos[0], s.campos[1], s.campos[2], s.look[0], s.look[1], s.look[2], s.aperture,
                     s.focus_dist, s.fov, s.max_depth if depth is None else depth, s.spp if spp is None else spp,
                     divisor, s.backtex], dtype=np.float32)


class Scene:
    """Host scene: objects, settings, textures, BVH (allobjects / nbvhtree / globals of the reference)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def load(cls, rts_path, texture_dir=""):
        """texture_dir: directory scanned for *ppm* entries; None = process cwd (reference behaviour),
        "" = none."""
        h = _VP()
        td = None if texture_dir is None else os.fsencode(texture_dir)
        _check(lib().dr_scene_load(os.fsencode(rts_path), td, C.byref(h)))
        return cls(h)

    @classmethod
    def load_binary(cls, rtsb_path):
        """A scene saved with save_binary(): objects, settings, textures and (if it was built) the BVH."""
        h = _VP()
        _check(lib().dr_scene_load_binary(os.fsencode(rtsb_path), C.byref(h)))
        return cls(h)

    def save_binary(self, rtsb_path):
        _check(lib().dr_scene_save_binary(self._h, os.fsencode(rtsb_path)))
        return rtsb_path

    @classmethod
    def from_arrays(cls, objects, settings=None, bvh=None, textures=()):
        """objects: OBJECT_DTYPE[N + 1]; bvh: BVH_DTYPE[2 * (N + 1)] or None; textures: uint8[h, w, 4] arrays."""
        objects = np.ascontiguousarray(objects, dtype=OBJECT_DTYPE)
        n = len(objects) - 1
        h = _VP()
        bp, bn = None, 0
        if bvh is not None:
            bvh = np.ascontiguousarray(bvh, dtype=BVH_DTYPE)
            bp, bn = _p(bvh), len(bvh)
        _check(lib().dr_scene_create_from_arrays(_p(objects), n, C.byref(settings) if settings is not None else None, bp, bn, C.byref(h)))
        sc = cls(h)
        for i, t in enumerate(textures):
            t = np.ascontiguousarray(t, dtype=np.uint8)
            rc = lib().dr_scene_add_texture(h, _p(t), t.shape[1], t.shape[0], ("texture%d" % i).encode())
            if rc < 0:
                _check(rc)
        return sc

    def close(self):
        if self._h:
            lib().dr_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def num_objects(self):
        return lib().dr_scene_num_objects(self._h)

    def objects(self):
        out = np.zeros(self.num_objects + 1, dtype=OBJECT_DTYPE)
        _check(lib().dr_scene_get_objects(self._h, _p(out)))
        return out

    def settings(self):
        s = DrSettings()
        _check(lib().dr_scene_get_settings(self._h, C.byref(s)))
        return s

    def set_settings(self, s):
        _check(lib().dr_scene_set_settings(self._h, C.byref(s)))

    def textures(self):
        res = []
        for i in range(lib().dr_scene_num_textures(self._h)):
            w, h = C.c_int(), C.c_int()
            _check(lib().dr_scene_texture_info(self._h, i, C.byref(w), C.byref(h)))
            a = np.zeros((h.value, w.value, 4), dtype=np.uint8)
            _check(lib().dr_scene_texture_data(self._h, i, _p(a)))
            res.append(a)
        return res

    def build_bvh(self, nthreads=0):
        _check(lib().dr_scene_build_bvh(self._h, nthreads))

    def bvh(self):
        n = lib().dr_scene_bvh_size(self._h)
        out = np.zeros(n, dtype=BVH_DTYPE)
        _check(lib().dr_scene_get_bvh(self._h, _p(out)))
        return out, lib().dr_scene_bvh_used(self._h)


class Context:
    """One GPU with a resident scene; render_frame() is the CudaStarter replacement."""

    def __init__(self, device=0):
        h = _VP()
        _check(lib().dr_context_create(device, C.byref(h)))
        self._h = h
        self.device = device

    def close(self):
        if self._h:
            lib().dr_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, scene):
        _check(lib().dr_context_upload_scene(self._h, scene._h))
        return self

    def set_stripe(self, mod, rem):
        _check(lib().dr_context_set_stripe(self._h, mod, rem))

    def set_traversal(self, mode):
        _check(lib().dr_context_set_traversal(self._h, mode))

    def set_option(self, name, value):
        """Tuning knob ("kernel", "batch_frames", "feedback", "occupancy", "schedule", ...: include/dogeray_amd.h); never changes a pixel."""
        _check(lib().dr_context_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int()
        _check(lib().dr_context_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def render_frame(self, settings13, W, H, background, frame_seed, download=True):
        """Returns int32[W, H, 3] indexed [x, y] (the reference's column-major int3 buffer) or None."""
        st = _f32(settings13)
        assert st.shape == (13,)
        out = np.empty((W, H, 3), dtype=np.int32) if download else None
        _check(lib().dr_render_frame(self._h, _p(st), W, H, float(background), int(frame_seed) & (2 ** 64 - 1),
                                     _p(out) if download else None))
        return out

    def accum_reset(self, W, H):
        _check(lib().dr_accum_reset(self._h, W, H))
        self._acc_shape = (W, H, 3)

    def render_accumulate(self, settings13, W, H, background, frame_seed, seed_stride, nframes):
        st = _f32(settings13)
        _check(lib().dr_render_accumulate(self._h, _p(st), W, H, float(background), int(frame_seed) & (2 ** 64 - 1),
                                          int(seed_stride) & (2 ** 64 - 1), nframes))

    def render_accumulate_async(self, settings13, W, H, background, frame_seed, seed_stride, nframes):
        """Queues the launches and returns (at most two batches in flight); synchronize() waits and updates stats()."""
        st = _f32(settings13)
        _check(lib().dr_render_accumulate_async(self._h, _p(st), W, H, float(background), int(frame_seed) & (2 ** 64 - 1),
                                                int(seed_stride) & (2 ** 64 - 1), nframes))

    def pipeline_submit(self, settings13, W, H, background, frame_seed, present_divide_by=0):
        """Queues one frame of the pipelined present loop (dr_pipeline_submit); returns its ticket.  The frame is rendered with the scene, stripe,
        traversal and options of this moment: upload, set_stripe, set_traversal, enable_counters and set_option apply to frames submitted after them."""
        st = _f32(settings13)
        t = C.c_uint64(0)
        _check(lib().dr_pipeline_submit(self._h, _p(st), W, H, float(background), int(frame_seed) & (2 ** 64 - 1), int(present_divide_by), C.byref(t)))
        return int(t.value)

    def pipeline_wait(self, ticket, want_image=False, in_place=False):
        """Waits for a submitted frame; with want_image the RGB8 image [H, W, 3] of exactly the frames up to that ticket (in_place: a
        read-only view of the library's pinned download buffer, valid until the next call that may launch a group of frames -- pipeline_submit, or
        any call ordered behind frames that are still held).  Every ticket handed out stays waitable until it has been waited for, however many
        groups have been launched since; the image of a presented frame is kept until then (at most 32 of them beyond the frames in flight:
        pipeline_submit raises ERR_INVALID rather than drop one).  A frame submitted without a present raises ERR_INVALID with want_image."""
        if not want_image:
            _check(lib().dr_pipeline_wait(self._h, int(ticket), None))
            return None
        W, H, _ = self._acc_shape
        if in_place:
            _check(lib().dr_pipeline_wait(self._h, int(ticket), None))
            ptr = _VP()
            _check(lib().dr_pipeline_image(self._h, int(ticket), C.byref(ptr)))
            buf = (C.c_uint8 * (W * H * 3)).from_address(ptr.value)
            img = np.frombuffer(buf, dtype=np.uint8).reshape(H, W, 3)
            img.flags.writeable = False
            return img
        img = np.empty((H, W, 3), dtype=np.uint8)
        _check(lib().dr_pipeline_wait(self._h, int(ticket), _p(img)))
        return img

    def render_accumulate_pipelined(self, settings13, W, H, background, frame_seed, seed_stride, nframes):
        st = _f32(settings13)
        _check(lib().dr_render_accumulate_pipelined(self._h, _p(st), W, H, float(background), int(frame_seed) & (2 ** 64 - 1),
                                                    int(seed_stride) & (2 ** 64 - 1), nframes))

    def synchronize(self):
        _check(lib().dr_context_synchronize(self._h))

    def stream_ptr(self):
        """The context's hipStream_t as an integer (torch.cuda.ExternalStream(ptr) orders torch work against it)."""
        p = _VP()
        _check(lib().dr_context_stream(self._h, C.byref(p)))
        return p.value or 0

    @contextlib.contextmanager
    def _torch_handshake(self):
        """The stream handshake of a call that reads or writes torch tensors, around the call: yields the torch device of this context's GPU; the
        library's stream waits for torch's current stream first, torch's current stream waits for the library's afterwards."""
        import torch
        dev = self._torch_device()
        lib_stream = torch.cuda.ExternalStream(self.stream_ptr(), device=dev)
        cur = torch.cuda.current_stream(dev)
        lib_stream.wait_stream(cur)
        yield dev
        cur.wait_stream(lib_stream)

    def _torch_device(self):
        import torch
        return torch.device("cuda", self.device if self.device is not None else torch.cuda.current_device())

    def _plane_read(self, read_fn, shape, dtype):
        """One of the accumulator's planes on the host: read_fn = dr_accum_read, dr_accum_history_read or dr_accum_moments_read."""
        out = np.empty(shape, dtype=dtype)
        _check(getattr(lib(), read_fn)(self._h, _p(out)))
        return out

    def _sized_read(self, stats_fn, dtype, items=lambda n: n):
        """An array the library sizes (dr_stats_cert_mask and its like): asked for its n first, then read into items(n) elements."""
        n = C.c_int()
        fn = getattr(lib(), stats_fn)
        _check(fn(self._h, None, 0, C.byref(n)))
        out = np.zeros(items(n.value), dtype=dtype)
        if len(out):
            _check(fn(self._h, out.ctypes.data_as(_VP), len(out), C.byref(n)))
        return out

    def accum_pack_stripe(self, slot):
        """Queues the packing of this context's stripe into library buffer `slot` (0/1); returns (device pointer, bytes)."""
        p, n = _VP(), C.c_uint64()
        _check(lib().dr_accum_pack_stripe(self._h, slot, C.byref(p), C.byref(n)))
        return p.value, n.value

    def accum_unpack_stripes(self, packed_ptr, rank_stride_bytes, world, first_rank=1, stream_ptr=None):
        _check(lib().dr_accum_unpack_stripes(self._h, C.c_void_p(packed_ptr), int(rank_stride_bytes), world, first_rank,
                                             C.c_void_p(stream_ptr) if stream_ptr else None))

    def accum_read(self):
        return self._plane_read("dr_accum_read", self._acc_shape, np.int32)

    def accum_present(self, divide_by):
        """uint8[H, W, 3] row-major image: clamp(acc / divide_by, 0, 255) (K:2287)."""
        W, H, _ = self._acc_shape
        out = np.empty((H, W, 3), dtype=np.uint8)
        _check(lib().dr_accum_present(self._h, divide_by, _p(out)))
        return out

    def accum_device_ptr(self):
        p, n = _VP(), C.c_uint64()
        _check(lib().dr_accum_device_ptr(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def enable_counters(self, on=True):
        _check(lib().dr_stats_enable_counters(self._h, 1 if on else 0))

    def stats_reset(self):
        _check(lib().dr_stats_reset(self._h))

    def stats(self):
        s = DrStats()
        _check(lib().dr_stats_get(self._h, C.byref(s)))
        return s.as_dict()

    def phase_counts(self, n=32):
        """The shade / refill phase's budget counters of the counting build (dr_stats_phase_counts)."""
        buf = (C.c_ulonglong * n)()
        _check(lib().dr_stats_phase_counts(self._h, buf, n))
        return [int(v) for v in buf]

    def cert_mask(self):
        """uint32 words of the last certified view's tile mask (dr_stats_cert_mask; bit set = the tile's camera rays keep the scene's margin),
        or an empty array when no certificate is in use."""
        return self._sized_read("dr_stats_cert_mask", np.uint32, lambda n: (n + 31) // 32)

    def cert_levels(self):
        """uint8 grades of the last certified view's tiles (dr_stats_cert_levels; 0 = the tile's camera rays keep the scene's margin, g >= 1 = they
        carry the margin of step g - 1 of the certificate's ladder), or an empty array when no certificate is in use."""
        return self._sized_read("dr_stats_cert_levels", np.uint8)

    def camera_entry(self):
        """int32 entry codes of the last certified view's tiles (dr_stats_camera_entry; wide record << 1 | is-leaf at which the tile's camera rays start,
        0 = the root, -1 = nothing can be seen from the tile), or an empty array when no table is in use."""
        return self._sized_read("dr_stats_camera_entry", np.int32)

    def sky_tiles(self):
        """(sky tiles, geometry tiles) of the last launch (dr_stats_sky_tiles): the tiles rendered without a walk (by sky_tiles_kernel, or by the persistent kernel's
        retiring waves: option "sky_tiles" 1 / 2) and the tiles left to the persistent kernel's queues; (0, 0) when the launch was not split (option "sky_tiles")."""
        n_sky, n_geometry = C.c_int(), C.c_int()
        _check(lib().dr_stats_sky_tiles(self._h, C.byref(n_sky), C.byref(n_geometry)))
        return n_sky.value, n_geometry.value

    def wave_log(self, max_waves=16384):
        """(n, 16) uint64: begin, queue-empty, end stamps (100 MHz ticks) and iterations after the queue was empty, per wave of the
        last persistent launch; needs set_option("wave_log", 1) before the launch."""
        out = np.zeros((max_waves, 16), dtype=np.uint64)
        n = C.c_int()
        _check(lib().dr_stats_wave_log(self._h, out.ctypes.data_as(C.POINTER(C.c_ulonglong)), max_waves, C.byref(n)))
        return out[:n.value]

    def pixel_cost(self, W, H, div=1, raw=False):
        """uint32 node steps per pixel of the last frame the persistent kernel recorded, over the renderer's grid of whole tiles -- gx = W // div // 8
        block columns of gy = H // div // 8 tiles (div: the preview divisor, settings13[11]; an unstriped context): shape (gx * 8, gy * 8), or with
        raw=True the flat gx * gy * 64 words as the feedback kernels read them (tile * 64 + lane).  An empty array: none recorded yet."""
        gx, gy = W // div // 8, H // div // 8
        out = np.zeros(gx * gy * 64, dtype=np.uint32)
        n = C.c_size_t()
        if out.size:
            _check(lib().dr_stats_pixel_cost(self._h, out.ctypes.data_as(C.POINTER(C.c_uint)), out.size, C.byref(n)))
        if n.value < out.size or out.size == 0:
            return np.zeros(0 if raw else (0, 0), dtype=np.uint32)
        if raw:
            return out
        return out.reshape(gx, gy, 8, 8).transpose(0, 2, 1, 3).reshape(gx * 8, gy * 8)

    def tile_order(self):
        """The live tile order (dr_stats_tile_order): None when no order is valid, else a dict with order int32[ntiles], region_start int32[17]
        and the last feedback pass's ntiles, regions, heavy_factor, split_steps, split_limit."""
        n = C.c_size_t()
        rs = np.zeros(2 * MAX_REGIONS + 1, dtype=np.int32)
        args = np.zeros(5, dtype=np.int32)
        _check(lib().dr_stats_tile_order(self._h, None, 0, C.byref(n), _p(rs), _p(args)))
        if n.value == 0:
            return None
        order = np.zeros(n.value, dtype=np.int32)
        _check(lib().dr_stats_tile_order(self._h, _p(order), order.size, C.byref(n), _p(rs), _p(args)))
        if n.value != order.size:
            return None
        return dict(order=order, region_start=rs, ntiles=int(args[0]), regions=int(args[1]), heavy_factor=int(args[2]), split_steps=int(args[3]),
                    split_limit=int(args[4]))

    def probe_trace(self, settings13, W, H, background, frame_seed, frames=2, variant=2):
        """Trace-only probe (dr_context_probe_trace): (rays per second, rays, results differing from the one-ray-per-lane walk)."""
        st = _f32(settings13)
        r = C.c_double(); n = C.c_uint64(); bad = C.c_uint64()
        _check(lib().dr_context_probe_trace(self._h, _p(st), W, H, float(background), int(frame_seed) & (2 ** 64 - 1), int(frames), int(variant), C.byref(r), C.byref(n), C.byref(bad)))
        return r.value, int(n.value), int(bad.value)

    def probe_rays(self, settings13, W, H, background, frame_seed):
        """The rays the trace-only probe walks (dr_context_probe_rays): one frame's rays in wavefront order -> (o float32[n, 3], d float32[n, 3])."""
        st = _f32(settings13)
        n = C.c_uint64()
        room = 2 * W * H              # one logging frame in the usual case; a frame with more rays than that is logged again with room for all
        while True:
            o, d = np.zeros((room, 3), np.float32), np.zeros((room, 3), np.float32)
            _check(lib().dr_context_probe_rays(self._h, _p(st), W, H, float(background), int(frame_seed) & (2 ** 64 - 1), _p(o), _p(d), room, C.byref(n)))
            if n.value <= room:
                return o[:n.value].copy(), d[:n.value].copy()
            room = n.value

    def probe_gather(self, hot_records=0, iters=2000):
        """Records/s of divergent, dependent 64-byte fetches from the resident wide array (bench.py roofline.gather)."""
        v = C.c_double()
        _check(lib().dr_context_probe_gather(self._h, int(hot_records), int(iters), C.byref(v)))
        return v.value

    def probe_frame_add(self, iters=10):
        """(plain add ms[iters], fused add ms[iters]) of the kernels that fold a frame into the accumulator, each launch timed alone
        (dr_context_probe_frame_add; the fused times are zeros without a second-moment plane)."""
        a, b = (C.c_double * iters)(), (C.c_double * iters)()
        _check(lib().dr_context_probe_frame_add(self._h, int(iters), a, b))
        return [float(v) for v in a], [float(v) for v in b]

    # ---- first-hit AOVs (dr_render_aov)
    def render_aov(self, settings13, W, H, window=None, channels=ALL, device=False):
        """First-hit buffers of the pinhole rays through the pixel centres (include/dogeray_amd.h dr_render_aov): a dict channel -> array
        [h, w] (t, distance, depth: float32; object, material: int32) or [h, w, k] (normal, albedo, dir: 3; uv: 2), row index = the
        renderer's y.  window (x0, y0, w, h) inside the pixel grid, None = all of it.  device=True: torch tensors on this context's GPU,
        written on the library's stream, which waits for torch's current stream first; torch's current stream waits for it afterwards."""
        return self._aov_window(settings13, W, H, window, channels, device, AOV_CHANNELS, DrAovBuffers(),
                                lambda st, win, bufs, dp: lib().dr_render_aov(self._h, _p(st), W, H, *win, C.byref(bufs), dp))

    def _aov_window(self, settings13, W, H, window, channels, device, known, bufs, call):
        """what render_aov and render_aov_lens share: the window, the channels' arrays, the call(st, window, bufs, device_pointers)"""
        st = _f32(settings13)
        assert st.shape == (13,)
        if window is None:
            gw, gh = pixel_grid(st, W, H)
            window = (0, 0, gw, gh)
        x0, y0, w, h = (int(v) for v in window)
        channels = tuple(channels)
        for k in channels:
            if k not in known:
                raise ValueError("unknown AOV channel %r (known: %s)" % (k, ", ".join(known)))
        shape = lambda k: (max(h, 0), max(w, 0)) + ((known[k][1],) if known[k][1] > 1 else ())
        out = {}
        with (self._torch_handshake() if device else contextlib.nullcontext()) as dev:
            for k in channels:
                out[k], address = _out_array(shape(k), known[k][0], dev)
                setattr(bufs, k, address)
            _check(call(st, (x0, y0, w, h), bufs, 1 if device else 0))
        return out

    # ---- lens-averaged AOVs (dr_render_aov_lens)
    def render_aov_lens(self, settings13, W, H, frame_seed, seed_stride, nframes, window=None, channels=None, device=False):
        """The first-hit buffers averaged over the renderer's own camera rays -- jittered, from a point on the lens -- of nframes frames seeded
        as render_accumulate(.., frame_seed, seed_stride, nframes) seeds them (include/dogeray_amd.h dr_render_aov_lens): a dict channel ->
        array [h, w] (coverage, depth, distance: float32; material: int32) or [h, w, 3] (normal, albedo).  nframes * spp must be 1 .. 256.
        window, channels (None: all of them) and device as render_aov's."""
        u64 = lambda v: int(v) & (2 ** 64 - 1)
        return self._aov_window(settings13, W, H, window, tuple(AOV_LENS_CHANNELS) if channels is None else channels, device, AOV_LENS_CHANNELS,
                                DrAovLensBuffers(), lambda st, win, bufs, dp: lib().dr_render_aov_lens(
                                    self._h, _p(st), W, H, *win, u64(frame_seed), u64(seed_stride), int(nframes), C.byref(bufs), dp))

    # ---- queries on the caller's lists (trace, radiance, trace_all, nearest): what they share
    def _list_query(self, inputs, out_spec, call):
        """The marshalling of a query on n caller items.  inputs: (name, array, shape tail, numpy dtype, torch dtype's name as the messages
        print it) each, an item's array [n] + tail; the arrays with the first one's tail are required and give n, the others may be None.
        out_spec: channel -> (numpy dtype, shape tail).  numpy arrays (or anything numpy converts) take the host path, torch tensors on this
        context's GPU (of the dtype named, contiguous) the device path: the library's stream waits for torch's current stream first, torch's
        current stream for it afterwards.  Every check is made before anything is launched.  call(ins, outs, n, device_pointers) makes the C
        call: ins name -> address or None, outs channel -> address.  Returns the dict channel -> array."""
        names = [i[0] for i in inputs]
        groups = []      # consecutive inputs of one tail are judged together: [o, d], [tmax]
        for i in inputs:
            if not groups or groups[-1][0][2] != i[2]:
                groups.append([])
            groups[-1].append(i)
        is_torch = [type(i[1]).__module__.split(".")[0] == "torch" for i in inputs if i[1] is not None]

        def shapes_of(group, arrays, n):
            if n is None:
                n = arrays[0].shape[0] if arrays[0].ndim == 2 else -1
            tail = tuple(group[0][2])
            if any(a is not None and tuple(a.shape) != (n,) + tail for a in arrays):      # (the wording is each method's own, kept)
                raise ValueError("%s must %sbe [n%s]" % (" and ".join(g[0] for g in group), "both " if len(group) > 1 and tail else "",
                                                         "".join(", %d" % t for t in tail)))
            return n

        if not any(is_torch):
            n, arr = None, {}
            for group in groups:
                for name, a, tail, npdt, _ in group:
                    arr[name] = np.ascontiguousarray(a, dtype=npdt) if a is not None or n is None else None
                n = shapes_of(group, [arr[g[0]] for g in group], n)
            out = {k: np.empty((n,) + tuple(tail), dtype=dt) for k, (dt, tail) in out_spec.items()}
            call({k: (a.ctypes.data if a is not None else None) for k, a in arr.items()}, {k: a.ctypes.data for k, a in out.items()}, n, 0)
            return out
        if not all(is_torch):
            raise TypeError("%s and %s must %s be numpy arrays or %s torch tensors" % ((", ".join(names[:-1]), names[-1]) + (("both",) * 2 if len(names) == 2 else ("all",) * 2)))
        import torch
        dev = self._torch_device()
        for name, a, _, _, tname in inputs:
            if a is None:
                continue
            if a.device != dev:
                raise ValueError("%s is on %s, not on this context's %s" % (name, a.device, dev))
            if a.dtype != getattr(torch, tname.split(".")[-1]):
                raise TypeError("%s must be %s, not %s" % (name, tname, a.dtype))
            if not a.is_contiguous():
                raise ValueError("%s must be contiguous" % name)
        n = None
        for group in groups:
            n = shapes_of(group, [g[1] for g in group], n)
        with self._torch_handshake():
            out = {k: _out_array((n,) + tuple(tail), dt, dev)[0] for k, (dt, tail) in out_spec.items()}
            call({name: (a.data_ptr() if a is not None else None) for name, a, _, _, _ in inputs}, {k: a.data_ptr() for k, a in out.items()}, n, 1)
        return out

    # ---- ray queries (dr_trace_rays)
    def trace(self, o, d, tmax=None, channels=("t", "object"), any_hit=False):
        """Closest hit or occlusion of the caller's rays (include/dogeray_amd.h dr_trace_rays): o, d [n, 3] float32 (d as traced, not normalised),
        tmax [n] or None (every ray 10000) -> a dict channel -> array [n] (t, distance: float32; object, material: int32, -1 on a miss) or [n, k]
        (normal, albedo: 3; uv: 2); any_hit=True -> {"occluded": int32[n]}, 1 where anything is hit at t <= tmax.  numpy inputs take the host
        path and return numpy arrays.  torch tensors on this context's GPU (float32, contiguous) take the device path and return torch tensors,
        written on the library's stream, which waits for torch's current stream first; torch's current stream waits for it afterwards.  Mixed or
        wrongly shaped inputs raise before anything is launched."""
        channels = ("occluded",) if any_hit else tuple(channels)
        for k in channels:
            if k != "occluded" and k not in TRACE_CHANNELS:
                raise ValueError("unknown trace channel %r (known: %s)" % (k, ", ".join(TRACE_CHANNELS)))
        if not any_hit and "occluded" in channels:
            raise ValueError("channel 'occluded' is what any_hit=True returns")
        if not channels:
            raise ValueError("no channel asked for")
        spec = lambda k: (np.int32, 1) if k == "occluded" else TRACE_CHANNELS[k]
        mode = TRACE_ANY if any_hit else TRACE_CLOSEST

        def call(ins, outs, n, device_pointers):
            rays, hits = DrRayBuffers(), DrHitBuffers()
            rays.origin, rays.dir, rays.tmax = ins["o"], ins["d"], ins["tmax"]
            for k, ptr in outs.items():
                setattr(hits, k, ptr)
            _check(lib().dr_trace_rays(self._h, mode, n, C.byref(rays), C.byref(hits), device_pointers))
        return self._list_query([("o", o, (3,), np.float32, "float32"), ("d", d, (3,), np.float32, "float32"), ("tmax", tmax, (), np.float32, "float32")],
                                {k: (spec(k)[0], (spec(k)[1],) if spec(k)[1] > 1 else ()) for k in channels}, call)

    # ---- radiance queries (dr_trace_radiance)
    def radiance(self, o, d, spp=1, max_depth=10, background=1.0, backtex=-1, seed=0, seeds=None, skip=None, channels=("radiance",)):
        """The light along the caller's rays (include/dogeray_amd.h dr_trace_radiance): o, d [n, 3] float32 (d as traced, not normalised), spp
        samples of raycolor each with depth max_depth; seeds uint64 [n] or None (ray i: seed + i), skip int32 [n] or None: generator outputs
        discarded after seeding -> a dict: "radiance" float32 [n, 3], the SUM of the samples (divide by spp for the mean), "bounces" int32 [n],
        the closest-hit queries of all samples.  numpy inputs take the host path and return numpy arrays; torch tensors on this context's GPU
        (o, d float32, seeds int64 holding the 64 bits, skip int32; contiguous) take the device path and return torch tensors -- Context.trace's
        convention.  Mixed or wrongly shaped inputs raise before anything is launched."""
        channels = tuple(channels)
        for k in channels:
            if k not in RADIANCE_CHANNELS:
                raise ValueError("unknown radiance channel %r (known: %s)" % (k, ", ".join(RADIANCE_CHANNELS)))
        if not channels:
            raise ValueError("no channel asked for")
        params = DrRadianceParams()
        _check(lib().dr_radiance_defaults(C.byref(params)))
        params.spp, params.max_depth, params.background, params.backtex = int(spp), int(max_depth), float(background), int(backtex)
        params.seed = int(seed) & (2 ** 64 - 1)

        def call(ins, outs, n, device_pointers):
            rays, res = DrRadianceRays(), DrRadianceOut()
            rays.origin, rays.dir, rays.seed, rays.skip = ins["o"], ins["d"], ins["seeds"], ins["skip"]
            for k, ptr in outs.items():
                setattr(res, k, ptr)
            _check(lib().dr_trace_radiance(self._h, n, C.byref(rays), C.byref(params), C.byref(res), device_pointers))
        return self._list_query([("o", o, (3,), np.float32, "torch.float32"), ("d", d, (3,), np.float32, "torch.float32"),
                                 ("seeds", seeds, (), np.uint64, "torch.int64"), ("skip", skip, (), np.int32, "torch.int32")],
                                {k: (RADIANCE_CHANNELS[k][0], (3,) if RADIANCE_CHANNELS[k][1] > 1 else ()) for k in channels}, call)

    # ---- all hits (dr_trace_all_hits)
    def trace_all(self, o, d, tmax=None, max_hits=4, kinds=("triangle", "sphere"), channels=("count", "t", "object")):
        """Every crossing of the caller's rays, the first max_hits in order (include/dogeray_amd.h dr_trace_all_hits): o, d [n, 3] float32 (d as
        traced, not normalised), tmax [n] or None (every ray 10000), K = max_hits in 0 .. ALLHITS_MAX, kinds: which primitives count -> a dict
        channel -> array: count int32 [n], the size of the whole set; t, distance float32 and object, material int32 [n, K]; normal, albedo
        [n, K, 3], uv [n, K, 2]; unused entries are t / object / material -1 and zeros.  max_hits=0 returns the count only.  numpy inputs take the
        host path and return numpy arrays; torch tensors on this context's GPU (float32, contiguous) take the device path and return torch
        tensors -- Context.trace's convention, stream hand-over included.  Bad arguments raise before anything is launched."""
        channels = tuple(channels)
        for k in channels:
            if k not in ALLHITS_CHANNELS:
                raise ValueError("unknown all-hits channel %r (known: %s)" % (k, ", ".join(ALLHITS_CHANNELS)))
        if not channels:
            raise ValueError("no channel asked for")
        K = int(max_hits)
        if K < 0 or K > ALLHITS_MAX:
            raise ValueError("max_hits must be in 0 .. %d" % ALLHITS_MAX)
        if K == 0 and channels != ("count",):
            raise ValueError("max_hits=0 returns the channel 'count' only")
        kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
        for k in kinds:
            if k not in ALLHITS_KINDS:
                raise ValueError("unknown kind %r (known: %s)" % (k, ", ".join(ALLHITS_KINDS)))
        if not kinds:
            raise ValueError("no kind asked for")
        params = DrAllHitsParams()
        _check(lib().dr_allhits_defaults(C.byref(params)))
        params.max_hits, params.kind_mask = K, sum(ALLHITS_KINDS[k] for k in set(kinds))
        tail = lambda k: () if ALLHITS_CHANNELS[k][1] == 0 else ((K,) if ALLHITS_CHANNELS[k][1] == 1 else (K, ALLHITS_CHANNELS[k][1]))

        def call(ins, outs, n, device_pointers):
            rays, res = DrRayBuffers(), DrAllHitsBuffers()
            rays.origin, rays.dir, rays.tmax = ins["o"], ins["d"], ins["tmax"]
            for k, ptr in outs.items():
                setattr(res, k, ptr)
            _check(lib().dr_trace_all_hits(self._h, n, C.byref(rays), C.byref(params), C.byref(res), device_pointers))
        return self._list_query([("o", o, (3,), np.float32, "float32"), ("d", d, (3,), np.float32, "float32"), ("tmax", tmax, (), np.float32, "float32")],
                                {k: (ALLHITS_CHANNELS[k][0], tail(k)) for k in channels}, call)

    def contains(self, points, directions=None):
        """Which points lie inside the resident scene's CLOSED triangle meshes: bool [n] for points [n, 3] (numpy in, numpy out; torch tensors on
        this context's GPU in, a torch tensor out).  Along each of three directions (CONTAINS_DIRECTIONS, or the caller's three: not along an
        axis of the mesh, no two orthogonal) the parity of the number of triangles the ray from the point crosses (trace_all, triangles only,
        max_hits=0) says inside (odd) or outside (even), and the majority of the three decides.  Three directions vote because a ray through an
        edge or a vertex that two triangles share may count 0 or 2 crossings there instead of 1.  Meant for watertight meshes: an open mesh has
        no inside, spheres are not solids for this test (hit_sphere reports an entry only), and a triangle too small or too edge-on for
        hit_tri's |a| >= 1e-4 at these direction lengths is not counted.  Points closer to the surface than about 1e-2 of its size may fall
        either way."""
        dirs = CONTAINS_DIRECTIONS if directions is None else tuple(tuple(float(x) for x in v) for v in directions)
        if len(dirs) != 3 or any(len(v) != 3 for v in dirs):
            raise ValueError("directions must be three 3-vectors")
        if type(points).__module__.split(".")[0] == "torch":
            import torch
            if points.dim() != 2 or points.shape[1] != 3:
                raise ValueError("points must be [n, 3]")
            votes = None
            for v in dirs:
                d = torch.tensor(v, dtype=torch.float32, device=points.device).expand(points.shape[0], 3).contiguous()
                odd = self.trace_all(points, d, max_hits=0, kinds=("triangle",), channels=("count",))["count"] & 1
                votes = odd if votes is None else votes + odd
            return votes >= 2
        points = _f32(points)
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError("points must be [n, 3]")
        votes = np.zeros(points.shape[0], np.int32)
        for v in dirs:
            d = np.ascontiguousarray(np.broadcast_to(np.array(v, np.float32), points.shape))
            votes += self.trace_all(points, d, max_hits=0, kinds=("triangle",), channels=("count",))["count"] & 1
        return votes >= 2

    # ---- point queries (dr_query_nearest)
    def nearest(self, p, rmax=None, channels=("distance", "object"), signed=False):
        """The nearest surface point of the resident scene to each point (dr_query_nearest; arguments, channels and paths: _nearest_unsigned
        below).  signed=True negates `distance` where Context.contains says the point lies inside a closed triangle mesh: the crossing parity that
        dr_query_nearest itself leaves out.  Only hits change sign (a miss stays -1, so ask with rmax=None when both can occur); every other
        channel, and the default signed=False, are the unsigned answer bit for bit."""
        out = self._nearest_unsigned(p, rmax, channels)
        if signed and "distance" in out:
            inside = self.contains(p)
            dist = out["distance"]
            if type(dist).__module__.split(".")[0] == "torch":
                import torch
                out["distance"] = torch.where(inside & (dist > 0), -dist, dist)
            else:
                out["distance"] = np.where(inside & (dist > 0), -dist, dist).astype(np.float32)
        return out

    def _nearest_unsigned(self, p, rmax=None, channels=("distance", "object")):
        """The nearest surface point of the resident scene to each point (include/dogeray_amd.h dr_query_nearest): p [n, 3] float32, rmax [n] or
        None (unbounded) -> a dict channel -> array [n] (distance, d2: float32; object, material: int32, -1 on a miss) or [n, k] (point: 3;
        uv: 2).  numpy inputs take the host path and return numpy arrays.  torch tensors on this context's GPU (float32, contiguous) take the
        device path and return torch tensors, written on the library's stream, which waits for torch's current stream first; torch's current
        stream waits for it afterwards.  Mixed or wrongly shaped inputs raise before anything is launched."""
        channels = tuple(channels)
        for k in channels:
            if k not in NEAREST_CHANNELS:
                raise ValueError("unknown nearest channel %r (known: %s)" % (k, ", ".join(NEAREST_CHANNELS)))
        if not channels:
            raise ValueError("no channel asked for")

        def call(ins, outs, n, device_pointers):
            pts, res = DrPointBuffers(), DrNearestBuffers()
            pts.point, pts.rmax = ins["p"], ins["rmax"]
            for k, ptr in outs.items():
                setattr(res, k, ptr)
            _check(lib().dr_query_nearest(self._h, n, C.byref(pts), C.byref(res), device_pointers))
        return self._list_query([("p", p, (3,), np.float32, "float32"), ("rmax", rmax, (), np.float32, "float32")],
                                {k: (NEAREST_CHANNELS[k][0], (NEAREST_CHANNELS[k][1],) if NEAREST_CHANNELS[k][1] > 1 else ()) for k in channels}, call)

    def pick(self, settings13, W, H, x, y):
        """Every channel of pixel (x, y) of the grid: t, distance, depth (float), object, material (int; -1 on a miss), normal, albedo,
        dir (3-tuples) and uv (2-tuple)."""
        a = self.render_aov(settings13, W, H, window=(x, y, 1, 1))
        return {k: (tuple(float(c) for c in v[0, 0]) if v.ndim == 3 else (int(v[0, 0]) if v.dtype == np.int32 else float(v[0, 0])))
                for k, v in a.items()}

    def autofocus(self, settings13, W, H, x=None, y=None):
        """A copy of settings13 with the focus distance [7] set to the depth of what pixel (x, y) sees (default: the centre of the grid) --
        the reference's Z/X keys (K:2471-2483) as one call.  On a miss settings13 comes back unchanged."""
        st = _f32(settings13).copy()
        gw, gh = pixel_grid(st, W, H)
        x = gw // 2 if x is None else x
        y = gh // 2 if y is None else y
        a = self.render_aov(st, W, H, window=(x, y, 1, 1), channels=("object", "depth"))
        if a["object"][0, 0] >= 0:
            st[7] = a["depth"][0, 0]
        return st

    # ---- denoiser (dr_accum_denoise)
    def denoise(self, settings13, W, H, divide_by, out="rgb8", device=False, **params):
        """The accumulator divided by divide_by, filtered by the AOV-guided a-trous denoiser (include/dogeray_amd.h dr_accum_denoise), in
        accum_present's layout: out="rgb8" -> uint8[H, W, 3], "f32" -> float32[H, W, 3] (0..255 units, unclamped), "both" -> (rgb8, f32).
        params: the fields of dr_denoise_params (iterations, sigma_luminance, normal_power_log2, sigma_depth, demodulate, material_stop), the
        rest at their defaults.  device=True: torch tensors on this context's GPU, with render_aov's stream handshake."""
        def prepare():
            p = denoise_params(**params)
            return lambda st, f, rgb, dp: lib().dr_accum_denoise(self._h, st, W, H, int(divide_by), C.byref(p), f, rgb, dp)
        return self._image_stage(settings13, W, H, out, device, prepare)

    def _image_stage(self, settings13, W, H, out, device, prepare):
        """What denoise and upscale share: the settings and `out` judged, then the stage's own parameters (prepare() judges them and returns call),
        the images allocated (numpy, or torch on this context's GPU inside the stream handshake) and call(settings13's address, f32's or None,
        rgb8's or None, device_pointers) -> the C call's status."""
        st = _f32(settings13)
        assert st.shape == (13,)
        if out not in ("rgb8", "f32", "both"):
            raise ValueError("out must be 'rgb8', 'f32' or 'both', not %r" % (out,))
        call = prepare()
        shape = (max(H, 0), max(W, 0), 3) if device else (H, W, 3)      # (a size below 0: numpy refuses it here, behind torch the library does)
        with (self._torch_handshake() if device else contextlib.nullcontext()) as dev:
            rgb, rgb_at = _out_array(shape, np.uint8, dev) if out in ("rgb8", "both") else (None, None)
            f, f_at = _out_array(shape, np.float32, dev) if out in ("f32", "both") else (None, None)
            _check(call(_p(st), f_at, rgb_at, 1 if device else 0))
        return rgb if out == "rgb8" else (f if out == "f32" else (rgb, f))

    # ---- upsampler (dr_accum_upscale)
    def upscale(self, settings13, W, H, divide_by, out="rgb8", device=False, prefilter=None, **params):
        """The accumulator rendered with settings13 (divisor settings13[11]) at full size (include/dogeray_amd.h dr_accum_upscale), in
        accum_present's layout: out="rgb8" -> uint8[H, W, 3], "f32" -> float32[H, W, 3] (0..255 units, unclamped), "both" -> (rgb8, f32).
        params: the fields of dr_upscale_params (mode = UPSCALE_GUIDED / UPSCALE_BLOCK, normal_power_log2, sigma_depth, demodulate,
        material_stop), the rest at their defaults.  prefilter: None, True (the denoiser's defaults, demodulate as here) or a dict of
        dr_denoise_params fields -- the a-trous filter then runs on the low grid first.  device=True: torch tensors on this context's GPU, with
        render_aov's stream handshake."""
        def prepare():
            p = upscale_params(**params)
            pre = None
            if prefilter is not None and prefilter is not False:
                d = {} if prefilter is True else dict(prefilter)
                d.setdefault("demodulate", p.demodulate)
                pre = C.byref(denoise_params(**d))
            return lambda st, f, rgb, dp: lib().dr_accum_upscale(self._h, st, W, H, int(divide_by), C.byref(p), pre, f, rgb, dp)
        return self._image_stage(settings13, W, H, out, device, prepare)

    # ---- temporal reprojection (dr_accum_reproject)
    def reproject(self, from_settings13, to_settings13, W, H, frames, **params):
        """Carries the accumulator from the view it was rendered in to another one (include/dogeray_amd.h dr_accum_reproject): frames = the
        frames added since the last accum_reset / reproject.  Afterwards the accumulator and its history plane (accum_history) belong to the new
        view and the caller's frame count starts again at 0.  params: the fields of dr_reproject_params (max_history, normal_cos,
        plane_tolerance, material_mask, sky), the rest at their defaults.  Returns the counts of grid pixels per class:
        {"pixels", "valid", "masked", "offscreen", "rejected"}."""
        a, b = _f32(from_settings13), _f32(to_settings13)
        assert a.shape == (13,) and b.shape == (13,)
        p = reproject_params(**params)
        r = DrReprojectResult()
        _check(lib().dr_accum_reproject(self._h, _p(a), _p(b), W, H, int(frames), C.byref(p), C.byref(r)))
        return {k: int(getattr(r, k)) for k, _ in DrReprojectResult._fields_}

    def accum_history(self):
        """int32[W, H] indexed [x, y]: the samples each pixel of the accumulator carries in addition to the frames added since the last
        reproject (all zeros when there is no history plane)."""
        return self._plane_read("dr_accum_history_read", self._acc_shape[:2], np.int32)

    # ---- second moments (option "moments", dr_accum_error)
    def accum_moments(self):
        """uint64[W, H] indexed [x, y]: the second-moment plane, the sum over the frames folded into the accumulator of their capped luma x 256,
        squared (all zeros when there is no plane: set_option("moments", 1) before accum_reset)."""
        return self._plane_read("dr_accum_moments_read", self._acc_shape[:2], np.uint64)

    def error(self, settings13, W, H, divide_by, tolerance, sigma=False, device=False):
        """The noise estimate of the accumulator (include/dogeray_amd.h dr_accum_error): a dict with the fields of dr_error_result -- pixels,
        estimated, above (estimated pixels whose sigma exceeds tolerance), sum_var_q16, bins[16] -- and, with sigma=True, "sigma": float32[H, W],
        the standard error of each pixel's displayed mean luma in 0..255 units (accum_present's layout; device=True: a torch tensor on this
        context's GPU, with render_aov's stream handshake)."""
        st = _f32(settings13)
        assert st.shape == (13,)
        r = DrErrorResult()
        device = bool(sigma and device)
        with (self._torch_handshake() if device else contextlib.nullcontext()) as dev:
            plane, plane_at = _out_array((max(H, 0), max(W, 0)), np.float32, dev) if sigma else (None, None)
            _check(lib().dr_accum_error(self._h, _p(st), W, H, int(divide_by), float(tolerance), plane_at, C.byref(r), 1 if device else 0))
        d = r.as_dict()
        if sigma:
            d["sigma"] = plane
        return d

    @staticmethod
    def converged(result, permille):
        """The stopping rule of render_until: the pixels above the tolerance and the pixels without an estimate are at most permille / 1000 of the grid."""
        return (result["above"] + (result["pixels"] - result["estimated"])) * 1000 <= permille * result["pixels"]

    def render_until(self, settings13, W, H, background, seed, stride, tolerance, permille, max_frames, check_every=8, frames_before=0):
        """Adds frames (seeds seed + k * stride) through the pipeline in chunks of check_every until the noise estimate says stop -- above +
        (pixels - estimated) <= permille * pixels / 1000 at `tolerance` -- or max_frames have been added.  Needs a second-moment plane.
        frames_before: frames already in the accumulator since the last accum_reset / reproject (they count in divide_by, not in max_frames).
        Returns (frames added, the last error() dict)."""
        assert check_every >= 1 and max_frames >= 1
        st = _f32(settings13)
        frames, result = 0, None
        while frames < max_frames:
            n = min(check_every, max_frames - frames)
            self.render_accumulate_pipelined(st, W, H, background, int(seed) + frames * int(stride), stride, n)
            frames += n
            result = self.error(st, W, H, frames_before + frames, tolerance)
            if self.converged(result, permille):
                break
        return frames, result

    # ---- adaptive sampling (dr_render_adaptive)
    def render_adaptive(self, settings13, W, H, background, frame_seed, seed_stride, nframes, divide_by, **params):
        """One adaptive pass (include/dogeray_amd.h dr_render_adaptive): nframes frames (seeds frame_seed + k * seed_stride) into the 8x8 tiles whose
        pixels still ask for samples -- n = history + divide_by below min_samples, or a noise estimate above tolerance -- and into no other pixel;
        params = fields of dr_adaptive_params.  Needs a second-moment plane.  Returns a dict with the fields of dr_adaptive_result."""
        st = _f32(settings13)
        assert st.shape == (13,)
        p = adaptive_params(**params)
        r = DrAdaptiveResult()
        _check(lib().dr_render_adaptive(self._h, _p(st), W, H, float(background), int(frame_seed) & (2 ** 64 - 1), int(seed_stride) & (2 ** 64 - 1),
                                        int(nframes), int(divide_by), C.byref(p), C.byref(r)))
        return {k: int(getattr(r, k)) for k, _ in DrAdaptiveResult._fields_}

    def adaptive_tiles(self):
        """uint8 flags of the last adaptive pass's tiles (dr_stats_adaptive_tiles; tile = block column * tile rows + row, 1 = rendered); empty
        before the first pass."""
        return self._sized_read("dr_stats_adaptive_tiles", np.uint8)

    def render_until_adaptive(self, settings13, W, H, background, seed, stride, tolerance, permille, max_frames, check_every=8, frames_before=0, **params):
        """render_until with the frames going where the noise is: max(min_samples - frames_before, 0) uniform frames through the pipeline, rounded up
        to check_every, then adaptive passes of check_every frames with consecutive seeds (params = the other fields of dr_adaptive_params) until
        the noise estimate says stop -- converged(error(...), permille) at `tolerance` --, a pass finds no active tile, or max_frames seeds have been
        used (the uniform frames count, as render_until counts frames; the last pass is cut to what is left).  Every pixel's own count is in the history plane from the first pass on: present / error / denoise with the
        uniform count frames_before + uniform frames.  Returns (uniform frames, passes, samples added by the passes, the last error() dict)."""
        assert check_every >= 1 and max_frames >= 1
        st = _f32(settings13)
        p = adaptive_params(tolerance=tolerance, **params)
        uniform = -(-max(p.min_samples - int(frames_before), 0) // check_every) * check_every
        if uniform:
            self.render_accumulate_pipelined(st, W, H, background, int(seed), stride, uniform)
        div = int(frames_before) + uniform
        frames, passes, samples = uniform, 0, 0
        result = self.error(st, W, H, div, tolerance)
        # (seeds are counted as render_until counts frames: the uniform frames and every pass's, max_frames in all, so that with every tile active
        # the two leave the same sums)
        while not self.converged(result, permille) and frames < max_frames:
            n = min(check_every, max_frames - frames)
            r = self.render_adaptive(st, W, H, background, int(seed) + frames * int(stride), stride, n, div, tolerance=tolerance, **params)
            passes += 1
            frames += n
            samples += r["samples_added"]
            if r["active_tiles"] == 0:
                break
            result = self.error(st, W, H, div, tolerance)
        return uniform, passes, samples, result

    # ---- known-answer hooks (tests): shapes and dtypes in KAT_HOOKS, the marshalling in kat_marshal
    def _kat(self, hook, arrays, head=(), mid=(), outs=lambda out: [_p(a) for a in out], n=None):
        """kat_marshal calling dr_kat_<hook>(context, *head, n, inputs, *mid, outs(output arrays))"""
        def call(n, ins, out):
            _check(getattr(lib(), "dr_kat_" + hook)(self._h, *head, n, *ins, *mid, *outs(out)))
        return kat_marshal(hook, arrays, call, n)

    def kat_rng(self, seed, n):
        return self._kat("rng", (), head=(seed,), n=n)[0]

    def kat_aabb(self, o, d, mn, mx):
        return self._kat("aabb", (o, d, mn, mx))

    def kat_tri(self, o, d, v0, v1, v2):
        return self._kat("tri", (o, d, v0, v1, v2))[0]

    def kat_node_planes(self, w, a, b):
        """(t_mix, t_cvt), 4 per word: the node test's plane arithmetic through v_fma_mix_f32 / through a conversion and an fma"""
        t1, t2 = self._kat("node_planes", (w, a, b))
        return t1.reshape(-1), t2.reshape(-1)

    def kat_sphere(self, o, d, c, r):
        return self._kat("sphere", (o, d, c, r))[0]

    def kat_optics(self, v, nrm, eta):
        return self._kat("optics", (v, nrm, eta))

    def kat_normal(self, obj_index, o, d, t):
        """getnormal K:703-773: (normal[n, 3] before the facing flip, texco[n, 3]) for hits of rays (o, d) at t on objects obj_index."""
        return self._kat("normal", (obj_index, o, d, t))

    def kat_hit(self, o, d, want_visits=False):
        out = self._kat("hit", (o, d), outs=lambda out: [_p(out[0]), _p(out[1]), _p(out[2]) if want_visits else None])
        return out if want_visits else out[:2]

    def kat_trace(self, o, d, variant=0):
        """kat_hit's rays through the lean build of the wide walk (dr_kat_trace): variant 0 one ray per lane, 1..7 the persistent trace-only kernel.
        (t, idx) in kat_hit's convention."""
        return self._kat("trace", (o, d), head=(int(variant),))

    # the shading step: where a hook returns "both forms" the arrays have a leading axis of 2 -- [0] the plain functions, [1] what the persistent kernel runs
    def kat_sample(self, seed, warm, kind):
        """dr_kat_sample: (point float32[2, n, 3], next uint32[2, n, 2]) -- rand_in_unit_sphere / rand_in_unit_disk, and rand_points_merged"""
        return self._kat("sample", (seed, warm, kind), outs=lambda out: [_p(out[0][0]), _p(out[1][0]), _p(out[0][1]), _p(out[1][1])])

    def kat_outside(self, d2):
        return self._kat("outside", (d2,))[0]

    def kat_tex(self, tex, u, v):
        return self._kat("tex", (tex, u, v))[0]

    def kat_bounce(self, obj_index, o, d, t, atten, seed, warm):
        """dr_kat_bounce: (alive int32[2, n], origin, direction, attenuation float32[2, n, 3], next uint32[2, n, 2]) -- shade_hit, and the split"""
        return self._kat("bounce", (obj_index, o, d, t, atten, seed, warm))

    def kat_miss(self, d, atten, backtex, background):
        return self._kat("miss", (d, atten), mid=(int(backtex), float(background)))[0]

    def kat_camera(self, settings13, W, H, frame_seed, stride, x, y, sample):
        """dr_kat_camera: (origin, dir float32[2, n, 3], next uint32[2, n, 2]) -- camera_ray, and the split"""
        st = _f32(settings13)
        return self._kat("camera", (x, y, sample), head=(_p(st), int(W), int(H), int(frame_seed) & (2 ** 64 - 1), int(stride) & 0xFFFFFFFF))

    def kat_store(self, color, spp):
        return self._kat("store", (color,), mid=(int(spp),))[0]

    def kat_store_merged(self, form, store_me, key, x, y, color, spp, acc, lds_in):
        """dr_kat_store_merged: the stores of whole waves (lane i of the arrays is lane i % 64 of wave i / 64) added to a copy of acc, int32[W, H, 3]
        -- form 0 store_pixel per lane, 1 store_pixels_merged, 2 store_pixels_merged_lds; lds_in: int32[waves, 7, 64], the waves' LDS rows before
        the store.  Returns (acc afterwards, the LDS rows afterwards).  Not in KAT_HOOKS: the accumulator goes in and out and no array but the
        lanes' has n items, so the shapes are judged here -- ValueError before the library is touched."""
        ins = [np.ascontiguousarray(a, dtype=dt) for a, dt in ((store_me, np.int32), (key, np.int32), (x, np.int32), (y, np.int32), (color, np.float32))]
        n = ins[0].shape[0]
        for a, name, tail in zip(ins, ("store_me", "key", "x", "y", "color"), ((), (), (), (), (3,))):
            if a.shape != (n,) + tail:
                raise ValueError("kat_store_merged: %s must be [%s]" % (name, ", ".join(["n"] + [str(k) for k in tail])))
        out = np.array(acc, dtype=np.int32, order="C")
        if out.ndim != 3 or out.shape[2] != 3:
            raise ValueError("kat_store_merged: acc must be [W, H, 3]")
        rows = np.ascontiguousarray(lds_in, dtype=np.int32)
        if rows.shape != (n // 64, 7, 64):
            raise ValueError("kat_store_merged: lds_in must be [n / 64, 7, 64]")
        after = np.zeros_like(rows)
        _check(lib().dr_kat_store_merged(self._h, int(form), n, *[_p(a) for a in ins], int(spp), out.shape[0], out.shape[1], _p(out), _p(rows), _p(after)))
        return out, after

    def kat_tile_feedback(self, pixel_cost, regions, heavy_factor, split_steps, split_limit, ntiles=None):
        """The feedback kernels on a flat uint32 plane of ntiles * 64 pixel costs (dr_kat_tile_feedback): (tile_cost uint32[ntiles],
        order int32[ntiles], region_start int32[17]); entries the kernels did not write are -1."""
        words = int(np.size(pixel_cost))
        n = words // 64 if ntiles is None else int(ntiles)
        if n >= 1 and words < n * 64:
            raise ValueError("pixel_cost holds fewer than ntiles * 64 words")

        def call(n, ins, out):
            _check(lib().dr_kat_tile_feedback(self._h, n, int(regions), int(heavy_factor), int(split_steps), int(split_limit), *ins, *[_p(a) for a in out]))
        return kat_marshal("tile_feedback", (pixel_cost,), call, n)

    def kat_order_split(self, kind, regions, order, region_start, key):
        """The kernel that splits a launch's tile order, on caller arrays (dr_kat_order_split): order int32[ntiles] or None (the identity),
        region_start int32[regions + 1 or more], key one entry per tile -- kind 0 the tiles' uint32 words, kind 1 byte flags -> (launch_order
        int32[ntiles], launch_region_start int32[17], dropped_list int32[ntiles], counts uint32[2] = dropped, kept); entries the kernel did not
        write are -1 (kind 1: all of dropped_list and counts)."""
        n = int(np.size(key))
        if order is not None and np.size(order) != n:
            raise ValueError("kat_order_split: order must be [n]")
        if np.size(region_start) < int(regions) + 1:
            raise ValueError("kat_order_split: region_start must hold regions + 1 entries")
        flags = np.ascontiguousarray(key, dtype=np.uint8) if int(kind) == 1 else None      # (the table states the words' type; flags are bytes)

        def call(n, ins, out):
            _check(lib().dr_kat_order_split(self._h, int(kind), n, int(regions), ins[0] if order is not None else None, ins[1],
                                            ins[2] if flags is None else _p(flags), *[_p(a) for a in out]))
        return kat_marshal("order_split", (np.zeros(0, np.int32) if order is None else order, region_start, np.zeros(0, np.uint32) if flags is not None else key),
                           call, n)


class Group:
    """dr_group: one process, one context + one host thread per GPU, stripes gathered to rank 0 (RCCL, or peer copies when
    ranks share a device).  devices: list of ordinals, e.g. [0, 1, 2, 3] -- or [0, 0, 0] to rehearse on one GPU."""

    def __init__(self, devices):
        devs = (C.c_int * len(devices))(*devices)
        h = _VP()
        _check(lib().dr_group_create(len(devices), devs, C.byref(h)))
        self._h = h
        self.size = len(devices)

    def close(self):
        if self._h:
            lib().dr_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def uses_rccl(self):
        return bool(lib().dr_group_uses_rccl(self._h))

    @property
    def rccl_ranks(self):
        """Ranks of the RCCL communicator (ncclCommCount); 0 with the copy transport."""
        return int(lib().dr_group_rccl_ranks(self._h))

    def context(self, rank):
        """Borrowed Context of one rank (owned by the group: do not close it)."""
        c = Context.__new__(Context)
        c._h = _VP(lib().dr_group_context(self._h, rank))
        c.device = None
        c.close = lambda: None
        return c

    def upload(self, scene):
        _check(lib().dr_group_upload_scene(self._h, scene._h))
        return self

    def accum_reset(self, W, H):
        _check(lib().dr_group_accum_reset(self._h, W, H))
        self._acc_shape = (W, H, 3)

    def render_accumulate(self, settings13, W, H, background, frame_seed, seed_stride, nframes, gather_every=0):
        st = _f32(settings13)
        _check(lib().dr_group_render_accumulate(self._h, _p(st), W, H, float(background), int(frame_seed) & (2 ** 64 - 1),
                                                int(seed_stride) & (2 ** 64 - 1), nframes, gather_every))

    def accum_read(self):
        c = self.context(0)
        c._acc_shape = self._acc_shape
        return c.accum_read()


class ProgressiveRenderer:
    """The present loop's render schedule (kernel.cu K:2154-2224), headless.

    iter 0..3: preview ladder at 1/8, 1/4, 1/2, 1/1 resolution into `outr` (iter 0 with the
    file's spp/depth, iter 1..3 with spp 1 / depth 2); iter >= 4: full-resolution frames with the
    file's spp/depth added to `outr`.  The displayed value is clamp(outr / (iter - pnum), 0, 255)
    with integer division (K:2287).  frame k uses seed seed_base + k * seed_stride.
    """

    LADDER = (8, 4, 2, 1)

    def __init__(self, ctx, scene_settings, seed_base=1, seed_stride=1000003):
        self.ctx = ctx
        self.s = scene_settings
        self.W, self.H = scene_settings.width, scene_settings.height
        self.seed_base, self.seed_stride = seed_base, seed_stride
        self.iter = 0
        self.frames_rendered = 0
        self._pnum = 3                  # iterations that do not count as samples of the accumulating phase: divide_by = iter - _pnum
        self.ctx.accum_reset(self.W, self.H)

    def _seed(self):
        return self.seed_base + self.frames_rendered * self.seed_stride

    def step(self):
        """One present-loop iteration.  Returns (td, divide_by) for display."""
        s, c = self.s, self.ctx
        if self.iter < 4:
            div = self.LADDER[self.iter]
            spp, depth = (s.spp, s.max_depth) if self.iter == 0 else (1, 2)
            st = pack_settings13(s, div, spp=spp, depth=depth)
            c.accum_reset(self.W, self.H)           # CudaStarter overwrites outr on these calls
            c.render_accumulate(st, self.W, self.H, s.background, self._seed(), 0, 1)
            pnum = self.iter
            td = div
        else:
            st = pack_settings13(s, 1)
            c.render_accumulate(st, self.W, self.H, s.background, self._seed(), 0, 1)
            pnum = self._pnum
            td = 1
        self.frames_rendered += 1
        self.iter += 1
        return td, self.iter - pnum

    def move_camera(self, scene_settings, reproject=True, **params):
        """Switches the renderer to other settings (a DrSettings of the same width and height: a camera or focus move).  reproject=True
        carries the image into the new view (Context.reproject with the divide_by of the last step(), params = fields of
        dr_reproject_params) and skips the preview ladder: the following step() calls add full-resolution frames and return divide_by
        1, 2, ... -- the frames since the move; the carried samples are in the history plane, which image() divides by as well.  Returns
        the counts Context.reproject returns.  reproject=False, or a move before the ladder is complete (there is no full-resolution image
        to carry yet): the reference's behaviour, the accumulator is reset and the ladder starts again; returns None."""
        assert (scene_settings.width, scene_settings.height) == (self.W, self.H), "move_camera cannot change the image size"
        if not reproject or self.iter < 4:
            self.s = scene_settings
            self.iter = 0
            self._pnum = 3
            self.ctx.accum_reset(self.W, self.H)
            return None
        self.ctx._acc_shape = (self.W, self.H, 3)
        counts = self.ctx.reproject(self.settings13(), pack_settings13(scene_settings, 1), self.W, self.H, self.iter - self._pnum, **params)
        self.s = scene_settings
        self.iter = max(self.iter, 5)   # past the ladder: settings13() is the full-resolution view from here on
        self._pnum = self.iter
        return counts

    def image(self, divide_by, denoise=None, upscale=None):
        """The displayed image: accum_present(divide_by); with denoise (True, or a dict of dr_denoise_params fields) the same image through
        Context.denoise, guided by the AOVs of the settings the last step() rendered with.  upscale (True, or a dict of dr_upscale_params
        fields): the last step()'s image at full size through Context.upscale -- a preview stage's td x td blocks (mode = UPSCALE_BLOCK) or
        its guided upsample; denoise then acts as the prefilter."""
        if upscale is not None and upscale is not False:
            params = {} if upscale is True else dict(upscale)
            pre = None if denoise is None or denoise is False else denoise
            return self.ctx.upscale(self.settings13(), self.W, self.H, divide_by, prefilter=pre, **params)
        if denoise is None or denoise is False:
            return self.ctx.accum_present(divide_by)
        params = {} if denoise is True else dict(denoise)
        return self.ctx.denoise(self.settings13(), self.W, self.H, divide_by, **params)

    def settings13(self):
        """The settings13 of the last step(): the preview ladder's divisor / spp / depth for the first four, the file's after them."""
        s = self.s
        if 1 <= self.iter <= 4:
            k = self.iter - 1
            return pack_settings13(s, self.LADDER[k], spp=s.spp if k == 0 else 1, depth=s.max_depth if k == 0 else 2)
        return pack_settings13(s, 1)

    def run_pipelined(self, nframes, on_image=None, in_flight=None):
        """The accumulating part of the loop (iter >= 4), `nframes` frames, pipelined (dr_pipeline_submit / dr_pipeline_wait): up to `in_flight` frames
        (default: two groups, 2 x option pipe_group) are queued before the oldest one's image is waited for.  on_image(iter, divide_by, rgb[H, W, 3])
        gets every displayed image, each exactly clamp(sum of the frames so far / divide_by, 0, 255)."""
        assert self.iter >= 4, "run the preview ladder (four step() calls) first"
        s, c = self.s, self.ctx
        c._acc_shape = (self.W, self.H, 3)
        st = pack_settings13(s, 1)
        if in_flight is None:
            in_flight = 2 * max(1, c.get_option("pipe_group"))
        pending = []
        for k in range(nframes):
            self.iter += 1
            div = self.iter - self._pnum
            pending.append((c.pipeline_submit(st, self.W, self.H, s.background, self._seed(), div), self.iter, div))
            self.frames_rendered += 1
            if len(pending) >= in_flight:
                t, it, dv = pending.pop(0)
                img = c.pipeline_wait(t, want_image=True)
                if on_image:
                    on_image(it, dv, img)
        for t, it, dv in pending:
            img = c.pipeline_wait(t, want_image=True)
            if on_image:
                on_image(it, dv, img)

    def run_until(self, tolerance, permille, max_frames, check_every=8):
        """The accumulating part of the loop (iter >= 4) until the noise estimate says stop (Context.render_until: the context needs
        set_option("moments", 1) before the renderer is made): at most max_frames more frames, in chunks of check_every.  Returns (frames added,
        the last Context.error dict); step() / image() go on from there."""
        assert self.iter >= 4, "run the preview ladder (four step() calls) first"
        s, c = self.s, self.ctx
        c._acc_shape = (self.W, self.H, 3)
        before = self.iter - self._pnum
        frames, result = c.render_until(pack_settings13(s, 1), self.W, self.H, s.background, self._seed(), self.seed_stride, tolerance, permille,
                                        max_frames, check_every=check_every, frames_before=before)
        self.frames_rendered += frames
        self.iter += frames
        return frames, result

    def run_until_adaptive(self, tolerance, permille, max_frames, check_every=8, **params):
        """run_until with adaptive passes (Context.render_until_adaptive; params = fields of dr_adaptive_params).  iter -- and with it the
        divide_by of step() / image() -- advances by the uniform frames only: what the passes add is counted per pixel in the history plane.
        Returns (uniform frames, passes, samples added by the passes, the last Context.error dict)."""
        assert self.iter >= 4, "run the preview ladder (four step() calls) first"
        s, c = self.s, self.ctx
        c._acc_shape = (self.W, self.H, 3)
        before = self.iter - self._pnum
        uniform, passes, samples, result = c.render_until_adaptive(pack_settings13(s, 1), self.W, self.H, s.background, self._seed(), self.seed_stride, tolerance,
                                                                   permille, max_frames, check_every=check_every, frames_before=before, **params)
        self.frames_rendered += min(uniform + passes * check_every, max_frames) if passes else uniform      # the seeds used: the last pass may be cut at max_frames
        self.iter += uniform
        return uniform, passes, samples, result
