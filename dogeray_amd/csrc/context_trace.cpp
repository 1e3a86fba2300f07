// Ray queries on caller rays (dr_trace_rays): the arguments judged, the plan, the launches of kernels_trace.hip.  The list's way in and out: context_query.cpp.
#include "context.hpp"

using namespace dr;

extern "C" {

int dr_trace_rays(dr_context* c, int mode, int64_t n, const dr_ray_buffers* rays, const dr_hit_buffers* hits, int device_pointers) {
  if (!c || !rays || !hits) { set_error("null argument"); return DR_ERR_INVALID; }
  if (mode != DR_TRACE_CLOSEST && mode != DR_TRACE_ANY) { set_error("trace: unknown mode " + std::to_string(mode)); return DR_ERR_INVALID; }
  if (n < 0 || n >= (int64_t)1 << 31) { set_error("trace: the ray count must be in [0, 2^31)"); return DR_ERR_INVALID; }
  if (!rays->origin || !rays->dir) { set_error("trace: null origin or dir"); return DR_ERR_INVALID; }
  const bool any = mode == DR_TRACE_ANY;
  // t, object, occluded: the trace kernel's; the others: the surface pass's
  const QueryIn in[3] = {{rays->origin, 3}, {rays->dir, 3}, {rays->tmax, 1}};
  const QueryOut out[8] = {{hits->t, 1, true}, {hits->object, 1, true}, {hits->occluded, 1, true}, {hits->distance, 1, true}, {hits->material, 1, true},
                           {hits->normal, 3, true}, {hits->uv, 2, true}, {hits->albedo, 3, true}};
  bool some = false, surface = false;
  for (int k = 0; k < 8; k++) { some = some || out[k].p; surface = surface || (k >= 3 && out[k].p); }
  if (any && (hits->t || hits->object || surface)) { set_error("trace: occlusion queries write `occluded` only"); return DR_ERR_INVALID; }
  if (!any && hits->occluded) { set_error("trace: `occluded` belongs to occlusion queries (DR_TRACE_ANY)"); return DR_ERR_INVALID; }
  if (!some) { set_error("trace: no output channel"); return DR_ERR_INVALID; }
  if (!c->walk) { set_error("no scene uploaded"); return DR_ERR_INVALID; }
  const TracePlan plan = plan_trace(n > 0 ? n : 1, c->traversal, c->wide != nullptr, c->num_cus, c->trace_kernel);
  if (plan.traversal == DR_TRAVERSAL_ORDERED && c->tree_depth > ORDERED_STACK) { set_error("tree too deep for ordered traversal"); return DR_ERR_SCENE; }
  if (n == 0) return DR_OK;
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before
  if (hits->object) DR_TRY(ensure_slot_to_orig(c));
  QueryIo io;
  DR_TRY(query_begin(c, (size_t)n, 1, in, 3, out, 8, device_pointers != 0, io));
  TraceLaunch T;
  memset(&T, 0, sizeof(T));
  T.n = (unsigned)n;
  T.slot_to_orig = c->slot_to_orig_dev;
  T.origin = (const float*)io.in[0]; T.dir = (const float*)io.in[1]; T.tmax = (const float*)io.in[2];
  T.t = (float*)io.out[0]; T.object = (int32_t*)io.out[1]; T.occluded = (int32_t*)io.out[2];
  T.distance = (float*)io.out[3]; T.material = (int32_t*)io.out[4]; T.normal = (float*)io.out[5]; T.uv = (float*)io.out[6]; T.albedo = (float*)io.out[7];
  if (surface) DR_TRY(query_scratch(c, (size_t)n, T.hit));
  if (plan.kernel == QUERY_KERNEL_PERSISTENT) DR_TRY(query_cursor(c, T.cursor));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  launch_trace(c->stream, P, plan, any, T);
  HIP_TRY(hipGetLastError());
  if (surface) {
    launch_trace_surface(c->stream, P, T);
    HIP_TRY(hipGetLastError());
  }
  return query_end(c, out, 8, device_pointers != 0, io);
}

}  // extern "C"
