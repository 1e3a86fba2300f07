// Radiance queries on caller rays (dr_trace_radiance): the arguments judged, the plan, the launch of kernels_radiance.hip.  The list's way in and out:
// context_query.cpp.
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
  if (!device_pointers && rays->skip)
    for (size_t i = 0; i < (size_t)n; i++)
      if (rays->skip[i] < 0) { set_error("radiance: skip[" + std::to_string(i) + "] is negative"); return DR_ERR_INVALID; }
  const RadiancePlan plan = plan_radiance(n > 0 ? n : 1, c->traversal, c->wide != nullptr, c->num_cus, c->radiance_kernel);
  if (plan.traversal == DR_TRAVERSAL_ORDERED && c->tree_depth > ORDERED_STACK) { set_error("tree too deep for ordered traversal"); return DR_ERR_SCENE; }
  if (n == 0) return DR_OK;
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before
  const QueryIn in[4] = {{rays->seed, 2}, {rays->origin, 3}, {rays->dir, 3}, {rays->skip, 1}};      // the 64-bit seeds first: query_begin's alignment rule
  const QueryOut ch[2] = {{out->radiance, 3, true}, {out->bounces, 1, true}};
  QueryIo io;
  DR_TRY(query_begin(c, (size_t)n, 1, in, 4, ch, 2, device_pointers != 0, io));
  RadianceLaunch R;
  memset(&R, 0, sizeof(R));
  R.n = (unsigned)n; R.spp = params->spp; R.base_seed = params->seed;
  R.seed = (const uint64_t*)io.in[0]; R.origin = (const float*)io.in[1]; R.dir = (const float*)io.in[2]; R.skip = (const int32_t*)io.in[3];
  R.radiance = (float*)io.out[0]; R.bounces = (int32_t*)io.out[1];
  if (plan.kernel == QUERY_KERNEL_PERSISTENT) DR_TRY(query_cursor(c, R.cursor));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  P.max_depth = params->max_depth; P.bgint = params->background; P.backtex = params->backtex;
  launch_radiance(c->stream, P, plan, R);
  HIP_TRY(hipGetLastError());
  return query_end(c, ch, 2, device_pointers != 0, io);
}

}  // extern "C"
