// Every crossing of a caller ray (dr_trace_all_hits): the arguments judged, the context's scratch, the launches of kernels_allhits.hip.
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
  // channel k: where the caller wants it and its words per entry (count: per ray; count, t, object: the walk kernel's; the others: the surface pass's)
  void* const want[8] = {out->count, out->t, out->object, out->material, out->distance, out->normal, out->uv, out->albedo};
  const int words[8] = {1, 1, 1, 1, 1, 3, 2, 3};
  bool some = false, listed = false, surface = false;
  for (int k = 0; k < 8; k++) { some = some || want[k]; listed = listed || (k >= 1 && want[k]); surface = surface || (k >= 3 && want[k]); }
  if (!some) { set_error("all hits: no output channel"); return DR_ERR_INVALID; }
  if (K == 0 && listed) { set_error("all hits: max_hits 0 returns `count` only"); return DR_ERR_INVALID; }
  if (!c->walk) { set_error("no scene uploaded"); return DR_ERR_INVALID; }
  if (n == 0) return DR_OK;
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before
  if (out->object && !c->slot_to_orig_dev) {
    DR_TRY(c->slot_to_orig_dev.alloc(c->slot_to_orig.size()));
    if (!c->slot_to_orig.empty())
      HIP_TRY(hipMemcpyAsync(c->slot_to_orig_dev, c->slot_to_orig.data(), c->slot_to_orig.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  }
  const AllHitsPlan plan = plan_allhits(n, c->wide != nullptr, c->num_cus, c->allhits_kernel);
  const size_t rays_n = (size_t)n;
  auto entries = [rays_n, K](int k) { return k == 0 ? rays_n : rays_n * (size_t)K; };
  if (surface) DR_TRY(c->allhits_hit.grow(2 * rays_n * (size_t)K, c->stream));
  if (plan.kernel == ALLHITS_KERNEL_PERSISTENT && !c->allhits_cursor) DR_TRY(c->allhits_cursor.alloc(1));
  AllHitsLaunch A;
  memset(&A, 0, sizeof(A));
  A.n = (unsigned)n;
  A.K = K; A.kind_mask = prm.kind_mask;
  A.slot_to_orig = c->slot_to_orig_dev;
  A.hit = surface ? c->allhits_hit.p : nullptr;
  A.cursor = c->allhits_cursor;
  void* dev[8] = {nullptr};
  if (device_pointers) {
    A.origin = rays->origin; A.dir = rays->dir; A.tmax = rays->tmax;
    for (int k = 0; k < 8; k++) dev[k] = want[k];
  } else {
    // staging: origin 3n | dir 3n | tmax n floats, then the wanted channels
    size_t bytes = rays_n * 7 * sizeof(float);
    for (int k = 0; k < 8; k++) if (want[k]) bytes += entries(k) * (size_t)words[k] * 4;
    DR_TRY(c->allhits_staging.grow(bytes, c->stream));
    float* const in = reinterpret_cast<float*>(c->allhits_staging.p);
    HIP_TRY(hipMemcpyAsync(in, rays->origin, rays_n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(in + 3 * rays_n, rays->dir, rays_n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (rays->tmax) HIP_TRY(hipMemcpyAsync(in + 6 * rays_n, rays->tmax, rays_n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    A.origin = in; A.dir = in + 3 * rays_n; A.tmax = rays->tmax ? in + 6 * rays_n : nullptr;
    size_t off = rays_n * 7 * sizeof(float);
    for (int k = 0; k < 8; k++) if (want[k]) { dev[k] = c->allhits_staging + off; off += entries(k) * (size_t)words[k] * 4; }
  }
  A.count = (int32_t*)dev[0]; A.t = (float*)dev[1]; A.object = (int32_t*)dev[2];
  A.material = (int32_t*)dev[3]; A.distance = (float*)dev[4]; A.normal = (float*)dev[5]; A.uv = (float*)dev[6]; A.albedo = (float*)dev[7];
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  if (plan.kernel == ALLHITS_KERNEL_PERSISTENT) HIP_TRY(hipMemsetAsync(c->allhits_cursor, 0, sizeof(unsigned), c->stream));      // a stale cursor would drop rays
  launch_allhits(c->stream, P, plan, A);
  HIP_TRY(hipGetLastError());
  if (surface) {
    launch_allhits_surface(c->stream, P, A);
    HIP_TRY(hipGetLastError());
  }
  if (device_pointers) return DR_OK;
  for (int k = 0; k < 8; k++)
    if (want[k]) HIP_TRY(hipMemcpyAsync(want[k], dev[k], entries(k) * (size_t)words[k] * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return DR_OK;
}

}  // extern "C"
