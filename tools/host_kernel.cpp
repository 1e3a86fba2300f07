// north_star's CPU baseline: "a host-C++ compile of the same kernel".  This translation unit compiles the product's OWN device functions
// (dogeray_amd/csrc/device_core.hpp with -DDR_HOST_BUILD: slab, tri_hit, sphere_hit, the wide and the threaded walk, surface_normal,
// shade_hit / shade_miss, Xorwow, camera_ray, render_pixel -- unchanged source, only the buffer loads become bounds-checked memcpys and the
// function qualifiers vanish) together with the product's host ingest (reader, BVH builder, lineariser, wide-walk builder) into
// tools/libhostkernel.so.  No device function's arithmetic is written here: the entries fill the product's parameter structs with host pointers and loop.
//
// It is TEST AND BENCH INFRASTRUCTURE: tests/test_host_kernel.py compares its frames with the oracle's pixel for pixel (a check of the
// kernel's arithmetic that needs no GPU) and bench.py reports it as cpu_baseline.kind "same-source" beside the oracle's "port".
// It is not linked into libdogeray_amd.so, which has no CPU path (dr_context_create fails without a GPU).
//
// The hk_* entries live in the headers of host_kernel/, included below in this order (one translation unit; tools/host_kernel.py binds every entry):
//   hk_api.h       C prototypes of the entries the stand-alone sanitizer drivers call, checked against the definitions here
//   hk_scene.hpp   the scene handle (hk_scene_load) and the one path from it to a loop: image(), fill_image, host_view, HostStack, with_closest,
//                  write_aov_channels, host_rows / host_grid; hk_last_error, hk_wide_info
//   hk_prims.hpp   primitives and generator checks on caller arrays: hk_check_uniform, hk_check_reject, hk_slab, hk_tri_hit, hk_hit_inputs, ...
//   hk_cert.hpp    the camera rays' certificate and entry table with their checks: hk_cert_check, hk_cert_levels, hk_camera_entry(_check), hk_wide_leaves
//   hk_plan.hpp    launch_plan.hpp, launch_state.hpp, device_sky.hpp and device_split.hpp: hk_persistent_plan, hk_trace_plan, ..., hk_order_begin, ..., hk_site_use, hk_sky_split, hk_sky_pixel, hk_sky_units_render
//   hk_pipeline.hpp pipeline_state.hpp: the pipelined present loop's ticket book and ordering plans, hk_pipeline_*
//   hk_kat.hpp     the shading step's known-answer hooks: hk_kat_sample .. hk_kat_store
//   hk_rays.hpp    caller rays: hk_hit, hk_trace, hk_ray_surface, hk_radiance, hk_allhits, hk_allhits_brute
//   hk_nearest.hpp caller points: hk_nearest, hk_nearest_brute, hk_nearest_prim(s), hk_nearest_records
//   hk_render.hpp  frames and first hits: hk_render (the measured baseline), hk_aov
//   hk_accum.hpp   the accumulator stages: hk_denoise, hk_upscale, hk_reproject, hk_moments_add, hk_error, hk_camera_block,
//                  hk_adaptive_select, hk_subset_split, hk_adaptive_add
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#define DR_HOST_BUILD 1
#include "../dogeray_amd/csrc/device_core.hpp"
#include "../dogeray_amd/csrc/device_trace.hpp"
#include "../dogeray_amd/csrc/device_allhits.hpp"
#include "../dogeray_amd/csrc/device_adaptive.hpp"
#include "../dogeray_amd/csrc/device_kat_shade.hpp"
#include "../dogeray_amd/csrc/device_denoise.hpp"
#include "../dogeray_amd/csrc/device_moments.hpp"
#include "../dogeray_amd/csrc/device_nearest.hpp"
#include "../dogeray_amd/csrc/device_radiance.hpp"
#include "../dogeray_amd/csrc/device_reproject.hpp"
#include "../dogeray_amd/csrc/device_sky.hpp"
#include "../dogeray_amd/csrc/device_split.hpp"
#include "../dogeray_amd/csrc/device_upscale.hpp"
#include "../dogeray_amd/csrc/launch_plan.hpp"
#include "../dogeray_amd/csrc/launch_state.hpp"
#include "../dogeray_amd/csrc/linearise.hpp"
#include "../dogeray_amd/csrc/params_host.hpp"
#include "../dogeray_amd/csrc/pipeline_state.hpp"
#include "../dogeray_amd/csrc/scene_host.hpp"

using namespace dr;

#include "host_kernel/hk_api.h"
#include "host_kernel/hk_scene.hpp"
#include "host_kernel/hk_prims.hpp"
#include "host_kernel/hk_cert.hpp"
#include "host_kernel/hk_plan.hpp"
#include "host_kernel/hk_pipeline.hpp"
#include "host_kernel/hk_kat.hpp"
#include "host_kernel/hk_rays.hpp"
#include "host_kernel/hk_nearest.hpp"
#include "host_kernel/hk_render.hpp"
#include "host_kernel/hk_accum.hpp"
