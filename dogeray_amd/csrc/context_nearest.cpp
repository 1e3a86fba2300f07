// Nearest-surface point queries (dr_query_nearest): the arguments judged, the context's scratch, the launches of kernels_nearest.hip.
#include "context.hpp"

using namespace dr;

extern "C" {

int dr_query_nearest(dr_context* c, int64_t n, const dr_point_buffers* pts, const dr_nearest_buffers* out, int device_pointers) {
  if (!c || !pts || !out) { set_error("null argument"); return DR_ERR_INVALID; }
  if (n < 0 || n >= (int64_t)1 << 31) { set_error("nearest: the query count must be in [0, 2^31)"); return DR_ERR_INVALID; }
  if (!pts->point) { set_error("nearest: null point"); return DR_ERR_INVALID; }
  // channel k: where the caller wants it and its words per query (distance, d2, object: the walk kernel's; the others: the finishing pass's)
  void* const want[6] = {out->distance, out->d2, out->object, out->material, out->point, out->uv};
  const int words[6] = {1, 1, 1, 1, 3, 2};
  bool some = false, finish = false;
  for (int k = 0; k < 6; k++) { some = some || want[k]; finish = finish || (k >= 3 && want[k]); }
  if (!some) { set_error("nearest: no output channel"); return DR_ERR_INVALID; }
  if (!c->walk) { set_error("no scene uploaded"); return DR_ERR_INVALID; }
  if (n == 0) return DR_OK;
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before
  if (out->object && !c->slot_to_orig_dev) {
    DR_TRY(c->slot_to_orig_dev.alloc(c->slot_to_orig.size()));
    if (!c->slot_to_orig.empty())
      HIP_TRY(hipMemcpyAsync(c->slot_to_orig_dev, c->slot_to_orig.data(), c->slot_to_orig.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  }
  const size_t q = (size_t)n;
  DR_TRY(c->nearest_key.grow(2 * q, c->stream));
  const NearestPlan plan = plan_nearest(n, c->wide != nullptr);
  NearestLaunch N;
  memset(&N, 0, sizeof(N));
  N.n = (unsigned)n;
  N.lmax = c->near_lmax;
  N.slot_to_orig = c->slot_to_orig_dev;
  N.key = c->nearest_key.p;
  void* dev[6] = {nullptr};
  if (device_pointers) {
    N.point = pts->point; N.rmax = pts->rmax;
    for (int k = 0; k < 6; k++) dev[k] = want[k];
  } else {
    // staging: point 3n | rmax n floats, then the wanted channels
    size_t bytes = q * 4 * sizeof(float);
    for (int k = 0; k < 6; k++) if (want[k]) bytes += q * (size_t)words[k] * 4;
    DR_TRY(c->nearest_staging.grow(bytes, c->stream));
    float* const in = reinterpret_cast<float*>(c->nearest_staging.p);
    HIP_TRY(hipMemcpyAsync(in, pts->point, q * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (pts->rmax) HIP_TRY(hipMemcpyAsync(in + 3 * q, pts->rmax, q * sizeof(float), hipMemcpyHostToDevice, c->stream));
    N.point = in; N.rmax = pts->rmax ? in + 3 * q : nullptr;
    size_t off = q * 4 * sizeof(float);
    for (int k = 0; k < 6; k++) if (want[k]) { dev[k] = c->nearest_staging + off; off += q * (size_t)words[k] * 4; }
  }
  N.distance = (float*)dev[0]; N.d2 = (float*)dev[1]; N.object = (int32_t*)dev[2];
  N.material = (int32_t*)dev[3]; N.qpoint = (float*)dev[4]; N.uv = (float*)dev[5];
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  launch_nearest(c->stream, P, plan, N);
  HIP_TRY(hipGetLastError());
  if (finish) {
    launch_nearest_finish(c->stream, P, plan, N);
    HIP_TRY(hipGetLastError());
  }
  if (device_pointers) return DR_OK;
  for (int k = 0; k < 6; k++)
    if (want[k]) HIP_TRY(hipMemcpyAsync(want[k], dev[k], q * (size_t)words[k] * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

}  // extern "C"
