// Radiance queries on caller rays (dr_trace_radiance): the arguments judged, the context's scratch, the launch of kernels_radiance.hip.
#include "context.hpp"

using namespace dr;

extern "C" {

int dr_radiance_defaults(dr_radiance_params* p) {
  if (!p) { set_error("null argument"); return DR_ERR_INVALID; }
  p->spp = 1; p->max_depth = 10; p->background = 1.0f; p->backtex = -1; p->seed = 0;
  return DR_OK;
}

int dr_trace_radiance(dr_context* c, int64_t n, const dr_radiance_rays* rays, const dr_radiance_params* params, const dr_radiance_out* out,
                      int device_pointers) {
  if (!c || !rays || !params || !out) { set_error("null argument"); return DR_ERR_INVALID; }
  if (n < 0 || n >= (int64_t)1 << 31) { set_error("radiance: the ray count must be in [0, 2^31)"); return DR_ERR_INVALID; }
  if (!rays->origin || !rays->dir) { set_error("radiance: null origin or dir"); return DR_ERR_INVALID; }
  if (!out->radiance && !out->bounces) { set_error("radiance: no output"); return DR_ERR_INVALID; }
  if (params->spp < 1) { set_error("radiance: spp must be >= 1"); return DR_ERR_INVALID; }
  if (params->max_depth < 1) { set_error("radiance: max_depth must be >= 1"); return DR_ERR_INVALID; }
  if (!c->walk) { set_error("no scene uploaded"); return DR_ERR_INVALID; }
  if (params->backtex >= c->n_tex) { set_error("backtex refers to a texture that is not loaded"); return DR_ERR_INVALID; }      // make_params' rule
  const size_t rays_n = (size_t)n;
  if (!device_pointers && rays->skip)
    for (size_t i = 0; i < rays_n; i++)
      if (rays->skip[i] < 0) { set_error("radiance: skip[" + std::to_string(i) + "] is negative"); return DR_ERR_INVALID; }
  const RadiancePlan plan = plan_radiance(n > 0 ? n : 1, c->traversal, c->wide != nullptr, c->num_cus, c->radiance_kernel);
  if (plan.traversal == DR_TRAVERSAL_ORDERED && c->tree_depth > ORDERED_STACK) { set_error("tree too deep for ordered traversal"); return DR_ERR_SCENE; }
  if (n == 0) return DR_OK;
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before
  if (plan.kernel == RADIANCE_KERNEL_PERSISTENT && !c->radiance_cursor) DR_TRY(c->radiance_cursor.alloc(1));
  RadianceLaunch R;
  memset(&R, 0, sizeof(R));
  R.n = (unsigned)n; R.spp = params->spp; R.base_seed = params->seed;
  R.cursor = c->radiance_cursor;
  uint8_t* stage = nullptr;
  size_t off_radiance = 0, off_bounces = 0;
  if (device_pointers) {
    R.origin = rays->origin; R.dir = rays->dir; R.seed = rays->seed; R.skip = rays->skip;
    R.radiance = out->radiance; R.bounces = out->bounces;
  } else {
    // staging: seed n words of 64 bits (first: its alignment) | origin 3n | dir 3n floats | skip n | radiance 3n | bounces n
    const size_t off_origin = rays_n * 8, off_dir = off_origin + rays_n * 12, off_skip = off_dir + rays_n * 12;
    off_radiance = off_skip + rays_n * 4; off_bounces = off_radiance + rays_n * 12;
    DR_TRY(c->radiance_staging.grow(off_bounces + rays_n * 4, c->stream));
    stage = c->radiance_staging.p;
    HIP_TRY(hipMemcpyAsync(stage + off_origin, rays->origin, rays_n * 12, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(stage + off_dir, rays->dir, rays_n * 12, hipMemcpyHostToDevice, c->stream));
    if (rays->seed) HIP_TRY(hipMemcpyAsync(stage, rays->seed, rays_n * 8, hipMemcpyHostToDevice, c->stream));
    if (rays->skip) HIP_TRY(hipMemcpyAsync(stage + off_skip, rays->skip, rays_n * 4, hipMemcpyHostToDevice, c->stream));
    R.origin = reinterpret_cast<const float*>(stage + off_origin); R.dir = reinterpret_cast<const float*>(stage + off_dir);
    R.seed = rays->seed ? reinterpret_cast<const uint64_t*>(stage) : nullptr;
    R.skip = rays->skip ? reinterpret_cast<const int32_t*>(stage + off_skip) : nullptr;
    R.radiance = out->radiance ? reinterpret_cast<float*>(stage + off_radiance) : nullptr;
    R.bounces = out->bounces ? reinterpret_cast<int32_t*>(stage + off_bounces) : nullptr;
  }
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  P.max_depth = params->max_depth; P.bgint = params->background; P.backtex = params->backtex;
  if (plan.kernel == RADIANCE_KERNEL_PERSISTENT) HIP_TRY(hipMemsetAsync(c->radiance_cursor, 0, sizeof(unsigned), c->stream));      // a stale cursor would drop rays
  launch_radiance(c->stream, P, plan, R);
  HIP_TRY(hipGetLastError());
  if (device_pointers) return DR_OK;
  if (out->radiance) HIP_TRY(hipMemcpyAsync(out->radiance, stage + off_radiance, rays_n * 12, hipMemcpyDeviceToHost, c->stream));
  if (out->bounces) HIP_TRY(hipMemcpyAsync(out->bounces, stage + off_bounces, rays_n * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

}  // extern "C"
