// Ray queries on caller rays (dr_trace_rays): the arguments judged, the context's scratch, the launches of kernels_trace.hip.
#include "context.hpp"

using namespace dr;

extern "C" {

int dr_trace_rays(dr_context* c, int mode, int64_t n, const dr_ray_buffers* rays, const dr_hit_buffers* hits, int device_pointers) {
  if (!c || !rays || !hits) { set_error("null argument"); return DR_ERR_INVALID; }
  if (mode != DR_TRACE_CLOSEST && mode != DR_TRACE_ANY) { set_error("trace: unknown mode " + std::to_string(mode)); return DR_ERR_INVALID; }
  if (n < 0 || n >= (int64_t)1 << 31) { set_error("trace: the ray count must be in [0, 2^31)"); return DR_ERR_INVALID; }
  if (!rays->origin || !rays->dir) { set_error("trace: null origin or dir"); return DR_ERR_INVALID; }
  const bool any = mode == DR_TRACE_ANY;
  // channel k: where the caller wants it and its words per ray (t, object, occluded: the trace kernel's; the others: the surface pass's)
  void* const want[8] = {hits->t, hits->object, hits->occluded, hits->distance, hits->material, hits->normal, hits->uv, hits->albedo};
  const int words[8] = {1, 1, 1, 1, 1, 3, 2, 3};
  bool some = false, surface = false;
  for (int k = 0; k < 8; k++) { some = some || want[k]; surface = surface || (k >= 3 && want[k]); }
  if (any && (hits->t || hits->object || surface)) { set_error("trace: occlusion queries write `occluded` only"); return DR_ERR_INVALID; }
  if (!any && hits->occluded) { set_error("trace: `occluded` belongs to occlusion queries (DR_TRACE_ANY)"); return DR_ERR_INVALID; }
  if (!some) { set_error("trace: no output channel"); return DR_ERR_INVALID; }
  if (!c->walk) { set_error("no scene uploaded"); return DR_ERR_INVALID; }
  const TracePlan plan = plan_trace(n > 0 ? n : 1, c->traversal, c->wide != nullptr, c->num_cus, c->trace_kernel);
  if (plan.traversal == DR_TRAVERSAL_ORDERED && c->tree_depth > ORDERED_STACK) { set_error("tree too deep for ordered traversal"); return DR_ERR_SCENE; }
  if (n == 0) return DR_OK;
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before
  if (hits->object && !c->slot_to_orig_dev) {
    DR_TRY(c->slot_to_orig_dev.alloc(c->slot_to_orig.size()));
    if (!c->slot_to_orig.empty())
      HIP_TRY(hipMemcpyAsync(c->slot_to_orig_dev, c->slot_to_orig.data(), c->slot_to_orig.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  }
  const size_t rays_n = (size_t)n;
  if (surface) DR_TRY(c->trace_hit.grow(2 * rays_n, c->stream));
  if (plan.kernel == TRACE_KERNEL_PERSISTENT && !c->trace_cursor) DR_TRY(c->trace_cursor.alloc(1));
  TraceLaunch T;
  memset(&T, 0, sizeof(T));
  T.n = (unsigned)n;
  T.slot_to_orig = c->slot_to_orig_dev;
  T.hit = surface ? c->trace_hit.p : nullptr;
  T.cursor = c->trace_cursor;
  void* dev[8] = {nullptr};
  if (device_pointers) {
    T.origin = rays->origin; T.dir = rays->dir; T.tmax = rays->tmax;
    for (int k = 0; k < 8; k++) dev[k] = want[k];
  } else {
    // staging: origin 3n | dir 3n | tmax n floats, then the wanted channels
    size_t bytes = rays_n * 7 * sizeof(float);
    for (int k = 0; k < 8; k++) if (want[k]) bytes += rays_n * (size_t)words[k] * 4;
    DR_TRY(c->trace_staging.grow(bytes, c->stream));
    float* const in = reinterpret_cast<float*>(c->trace_staging.p);
    HIP_TRY(hipMemcpyAsync(in, rays->origin, rays_n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(in + 3 * rays_n, rays->dir, rays_n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (rays->tmax) HIP_TRY(hipMemcpyAsync(in + 6 * rays_n, rays->tmax, rays_n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    T.origin = in; T.dir = in + 3 * rays_n; T.tmax = rays->tmax ? in + 6 * rays_n : nullptr;
    size_t off = rays_n * 7 * sizeof(float);
    for (int k = 0; k < 8; k++) if (want[k]) { dev[k] = c->trace_staging + off; off += rays_n * (size_t)words[k] * 4; }
  }
  T.t = (float*)dev[0]; T.object = (int32_t*)dev[1]; T.occluded = (int32_t*)dev[2];
  T.distance = (float*)dev[3]; T.material = (int32_t*)dev[4]; T.normal = (float*)dev[5]; T.uv = (float*)dev[6]; T.albedo = (float*)dev[7];
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  if (plan.kernel == TRACE_KERNEL_PERSISTENT) HIP_TRY(hipMemsetAsync(c->trace_cursor, 0, sizeof(unsigned), c->stream));      // a stale cursor would drop rays
  launch_trace(c->stream, P, plan, any, T);
  HIP_TRY(hipGetLastError());
  if (surface) {
    launch_trace_surface(c->stream, P, T);
    HIP_TRY(hipGetLastError());
  }
  if (device_pointers) return DR_OK;
  for (int k = 0; k < 8; k++)
    if (want[k]) HIP_TRY(hipMemcpyAsync(want[k], dev[k], rays_n * (size_t)words[k] * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

}  // extern "C"
