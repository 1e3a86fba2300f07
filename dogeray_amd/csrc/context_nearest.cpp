// Nearest-surface point queries (dr_query_nearest): the arguments judged, the plan, the launches of kernels_nearest.hip.  The list's way in and out:
// context_query.cpp.
#include "context.hpp"

using namespace dr;

extern "C" {

int dr_query_nearest(dr_context* c, int64_t n, const dr_point_buffers* pts, const dr_nearest_buffers* out, int device_pointers) {
  if (!c || !pts || !out) { set_error("null argument"); return DR_ERR_INVALID; }
  if (n < 0 || n >= (int64_t)1 << 31) { set_error("nearest: the query count must be in [0, 2^31)"); return DR_ERR_INVALID; }
  if (!pts->point) { set_error("nearest: null point"); return DR_ERR_INVALID; }
  // distance, d2, object: the walk kernel's; the others: the finishing pass's
  const QueryIn in[2] = {{pts->point, 3}, {pts->rmax, 1}};
  const QueryOut ch[6] = {{out->distance, 1, true}, {out->d2, 1, true}, {out->object, 1, true}, {out->material, 1, true}, {out->point, 3, true}, {out->uv, 2, true}};
  bool some = false, finish = false;
  for (int k = 0; k < 6; k++) { some = some || ch[k].p; finish = finish || (k >= 3 && ch[k].p); }
  if (!some) { set_error("nearest: no output channel"); return DR_ERR_INVALID; }
  if (!c->walk) { set_error("no scene uploaded"); return DR_ERR_INVALID; }
  if (n == 0) return DR_OK;
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before
  if (out->object) DR_TRY(ensure_slot_to_orig(c));
  const NearestPlan plan = plan_nearest(n, c->wide != nullptr);
  QueryIo io;
  DR_TRY(query_begin(c, (size_t)n, 1, in, 2, ch, 6, device_pointers != 0, io));
  NearestLaunch N;
  memset(&N, 0, sizeof(N));
  N.n = (unsigned)n;
  N.lmax = c->near_lmax;
  N.slot_to_orig = c->slot_to_orig_dev;
  N.point = (const float*)io.in[0]; N.rmax = (const float*)io.in[1];
  N.distance = (float*)io.out[0]; N.d2 = (float*)io.out[1]; N.object = (int32_t*)io.out[2];
  N.material = (int32_t*)io.out[3]; N.qpoint = (float*)io.out[4]; N.uv = (float*)io.out[5];
  DR_TRY(query_scratch(c, (size_t)n, N.key));      // (always: the walk kernel writes its keys whatever is asked for)
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  launch_nearest(c->stream, P, plan, N);
  HIP_TRY(hipGetLastError());
  if (finish) {
    launch_nearest_finish(c->stream, P, plan, N);
    HIP_TRY(hipGetLastError());
  }
  return query_end(c, ch, 6, device_pointers != 0, io);
}

}  // extern "C"
