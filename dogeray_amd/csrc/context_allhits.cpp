// Every crossing of a caller ray (dr_trace_all_hits): the arguments judged, the plan, the launches of kernels_allhits.hip.  The list's way in and out:
// context_query.cpp.
#include "context.hpp"

using namespace dr;

extern "C" {

int dr_allhits_defaults(dr_allhits_params* p) {
  if (!p) { set_error("null argument"); return DR_ERR_INVALID; }
  p->max_hits = 4; p->kind_mask = DR_ALLHITS_TRIANGLES | DR_ALLHITS_SPHERES;
  return DR_OK;
}

int dr_trace_all_hits(dr_context* c, int64_t n, const dr_ray_buffers* rays, const dr_allhits_params* params, const dr_allhits_buffers* out, int device_pointers) {
  if (!c || !rays || !out) { set_error("null argument"); return DR_ERR_INVALID; }
  dr_allhits_params prm;
  dr_allhits_defaults(&prm);
  if (params) prm = *params;
  if (n < 0 || n >= (int64_t)1 << 31) { set_error("all hits: the ray count must be in [0, 2^31)"); return DR_ERR_INVALID; }
  if (!rays->origin || !rays->dir) { set_error("all hits: null origin or dir"); return DR_ERR_INVALID; }
  if (prm.max_hits < 0 || prm.max_hits > DR_ALLHITS_MAX) { set_error("all hits: max_hits must be in [0, " + std::to_string(DR_ALLHITS_MAX) + "]"); return DR_ERR_INVALID; }
  if (prm.kind_mask <= 0 || prm.kind_mask > (DR_ALLHITS_TRIANGLES | DR_ALLHITS_SPHERES)) { set_error("all hits: kind_mask names no kind, or an unknown one"); return DR_ERR_INVALID; }
  const int K = prm.max_hits;
  // count: per ray, the others per entry; count, t, object: the walk kernel's; the others: the surface pass's
  const QueryIn in[3] = {{rays->origin, 3}, {rays->dir, 3}, {rays->tmax, 1}};
  const QueryOut ch[8] = {{out->count, 1, true}, {out->t, 1, false}, {out->object, 1, false}, {out->material, 1, false}, {out->distance, 1, false},
                          {out->normal, 3, false}, {out->uv, 2, false}, {out->albedo, 3, false}};
  bool some = false, listed = false, surface = false;
  for (int k = 0; k < 8; k++) { some = some || ch[k].p; listed = listed || (k >= 1 && ch[k].p); surface = surface || (k >= 3 && ch[k].p); }
  if (!some) { set_error("all hits: no output channel"); return DR_ERR_INVALID; }
  if (K == 0 && listed) { set_error("all hits: max_hits 0 returns `count` only"); return DR_ERR_INVALID; }
  if (!c->walk) { set_error("no scene uploaded"); return DR_ERR_INVALID; }
  if (n == 0) return DR_OK;
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before
  if (out->object) DR_TRY(ensure_slot_to_orig(c));
  const AllHitsPlan plan = plan_allhits(n, c->wide != nullptr, c->num_cus, c->allhits_kernel);
  QueryIo io;
  DR_TRY(query_begin(c, (size_t)n, (size_t)K, in, 3, ch, 8, device_pointers != 0, io));
  AllHitsLaunch A;
  memset(&A, 0, sizeof(A));
  A.n = (unsigned)n;
  A.K = K; A.kind_mask = prm.kind_mask;
  A.slot_to_orig = c->slot_to_orig_dev;
  A.origin = (const float*)io.in[0]; A.dir = (const float*)io.in[1]; A.tmax = (const float*)io.in[2];
  A.count = (int32_t*)io.out[0]; A.t = (float*)io.out[1]; A.object = (int32_t*)io.out[2];
  A.material = (int32_t*)io.out[3]; A.distance = (float*)io.out[4]; A.normal = (float*)io.out[5]; A.uv = (float*)io.out[6]; A.albedo = (float*)io.out[7];
  if (surface) DR_TRY(query_scratch(c, (size_t)n * (size_t)K, A.hit));
  if (plan.kernel == QUERY_KERNEL_PERSISTENT) DR_TRY(query_cursor(c, A.cursor));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  launch_allhits(c->stream, P, plan, A);
  HIP_TRY(hipGetLastError());
  if (surface) {
    launch_allhits_surface(c->stream, P, A);
    HIP_TRY(hipGetLastError());
  }
  return query_end(c, ch, 8, device_pointers != 0, io);
}

}  // extern "C"
