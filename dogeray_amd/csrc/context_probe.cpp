// Measurement probes (dr_context_probe_*) and the known-answer hooks of single device functions (dr_kat_*).
#include <deque>
#include <initializer_list>
#include <map>
#include <utility>

#include "context.hpp"

using namespace dr;

extern "C" {

int dr_context_probe_frame_add(dr_context* c, int iters, double* plain_ms, double* fused_ms) {
  if (!c || iters < 1 || !plain_ms || !fused_ms) { set_error("bad argument"); return DR_ERR_INVALID; }
  if (!c->accum) { set_error("no accumulator: call dr_accum_reset(W, H) first"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));
  const size_t npix = (size_t)c->accW * c->accH, elems = npix * 3;
  DR_TRY(c->frame.grow(elems, c->stream));
  HIP_TRY(hipMemsetAsync(c->frame, 0, elems * sizeof(int32_t), c->stream));      // a black frame: neither the sums nor the plane change
  for (int k = 0; k < 2 * iters; k++) {
    const bool fused = k >= iters;
    float ms = 0;
    if (!fused || c->m2) {
      HIP_TRY(hipEventRecord(c->ev0, c->stream));
      if (fused) launch_moments_add(c->stream, c->accum, c->frame, c->m2, npix);
      else launch_frame_add(c->stream, c->accum, c->frame, elems);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(c->ev1, c->stream));
      HIP_TRY(hipEventSynchronize(c->ev1));
      HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    }
    (fused ? fused_ms : plain_ms)[k % iters] = (double)ms;
  }
  return DR_OK;
}

int dr_context_probe_gather(dr_context* c, uint32_t hot_records, int iters, double* records_per_s) {
  if (!c || !records_per_s || iters < 1) { set_error("bad argument"); return DR_ERR_INVALID; }
  if (!c->wide) { set_error("no wide walk resident"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // timed behind the frames submitted before, not beside them
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  const unsigned total = (unsigned)(c->wide_bytes / 64);
  const unsigned nrec = (hot_records == 0 || hot_records > total) ? total : hot_records;
  DevMem<unsigned> out;
  DR_TRY(out.alloc(1));
  const int blocks = c->num_cus * 5;
  launch_gather_probe(c->stream, P, blocks, nrec, iters / 8 + 1, out.p);      // warm-up
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  launch_gather_probe(c->stream, P, blocks, nrec, iters, out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  HIP_TRY(hipEventSynchronize(c->ev1));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  *records_per_s = (double)blocks * 256.0 * (double)iters / ((double)ms * 1e-3);
  return DR_OK;
}

// The rays of ONE frame, as a per-bounce wavefront would hold them: the counting build writes every ray a path starts to slot bounce * pixels + pixel (tile
// order); empty slots (paths that had ended) are squeezed out on the host.  packed: 8 floats per ray -- origin, pad, direction, pad.  Resets the accumulator.
static int log_frame_rays(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed, size_t max_rays, std::vector<float>& packed) {
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(dr_accum_reset(c, W, H));
  RenderParams Pv;
  DR_TRY(make_params(c, c->own_site(), settings13, W, H, background, frame_seed, Pv, 1));
  const size_t npix = (size_t)Pv.ncols * Pv.gy * 64;
  const size_t slots = npix * (size_t)(Pv.max_depth > 0 ? Pv.max_depth : 1);
  if (slots > max_rays) { set_error("too many rays"); return DR_ERR_INVALID; }
  DevMem<float> raw;
  DR_TRY(raw.alloc(slots * 8));
  HIP_TRY(hipMemset(raw.p, 0, slots * 8 * sizeof(float)));
  const bool was_counting = c->count;
  unsigned long long ctl[3] = {0ull, (unsigned long long)(uintptr_t)raw.p, (unsigned long long)slots};      // STAT_LOG_RAYS, STAT_LOG_PTR, STAT_LOG_ROOM
  HIP_TRY(hipMemcpy(c->counters + STAT_LOG_RAYS, ctl, sizeof(ctl), hipMemcpyHostToDevice));
  c->count = true;
  const int rc = dr_render_accumulate(c, settings13, W, H, background, frame_seed, 1000003, 1);
  c->count = was_counting;
  const unsigned long long off[2] = {0ull, 0ull};
  HIP_TRY(hipMemcpy(c->counters + STAT_LOG_PTR, off, sizeof(off), hipMemcpyHostToDevice));
  if (rc != DR_OK) return rc;
  std::vector<float> host(slots * 8);
  DR_TRY(raw.get(host.data(), host.size()));
  packed.clear();
  packed.reserve(host.size() / 2);
  for (size_t k = 0; k < slots; k++) {
    const float* r = &host[k * 8];
    if (r[4] != 0.0f || r[5] != 0.0f || r[6] != 0.0f || r[4] != r[4]) packed.insert(packed.end(), r, r + 8);      // a direction was written
  }
  return DR_OK;
}

int dr_context_probe_trace(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed, int frames, int variant,
                           double* rays_per_s, uint64_t* n_rays, uint64_t* mismatches) {
  if (!c || !settings13 || !rays_per_s || !n_rays || !mismatches || frames < 1 || variant < 0) { set_error("bad argument"); return DR_ERR_INVALID; }
  if (!c->wide || traversal_of(c) != DR_TRAVERSAL_WIDE || !uses_persistent(c)) { set_error("the trace probe needs the wide walk and the persistent kernel"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before
  // 1. the rays of one frame in wavefront order (log_frame_rays); `frames` copies of the list make the probe's launch long enough to time
  std::vector<float> packed;
  DR_TRY(log_frame_rays(c, settings13, W, H, background, frame_seed, 0x7fffffffull / (size_t)frames, packed));
  DevMem<float> log; DevMem<unsigned> cursor; DevMem<unsigned> out, ref;
  const size_t per_frame = packed.size() / 8;
  const unsigned n = (unsigned)(per_frame * (size_t)frames);
  *n_rays = per_frame;
  if (n == 0) { *rays_per_s = 0; *mismatches = 0; return DR_OK; }
  DR_TRY(log.alloc((size_t)n * 8));
  for (int f = 0; f < frames; f++) HIP_TRY(hipMemcpy(log.p + (size_t)f * per_frame * 8, packed.data(), per_frame * 8 * sizeof(float), hipMemcpyHostToDevice));
  DR_TRY(cursor.alloc(1)); DR_TRY(out.alloc((size_t)n * 2)); DR_TRY(ref.alloc((size_t)n * 2));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  // 2. the probe, timed (one warm-up, then the best of three)
  float best = 1e30f;
  for (int rep = 0; rep < 4; rep++) {
    HIP_TRY(hipMemsetAsync(cursor.p, 0, sizeof(unsigned), c->stream));
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    launch_trace_probe(c->stream, P, c->num_cus, variant, log.p, n, cursor.p, out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (rep > 0 && ms < best) best = ms;
  }
  *rays_per_s = (double)n / ((double)best * 1e-3);
  // 3. every result against the one-ray-per-lane walk
  launch_trace_probe(c->stream, P, c->num_cus, 0, log.p, n, cursor.p, ref.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::vector<unsigned> a((size_t)n * 2), b((size_t)n * 2);
  DR_TRY(out.get(a.data(), a.size())); DR_TRY(ref.get(b.data(), b.size()));
  uint64_t bad = 0;
  for (size_t i = 0; i < a.size(); i++) bad += a[i] != b[i];
  *mismatches = bad;
  return DR_OK;
}

int dr_context_probe_rays(dr_context* c, const float settings13[13], int W, int H, float background, uint64_t frame_seed, float* origin, float* dir,
                          uint64_t capacity, uint64_t* n_rays) {
  if (!c || !settings13 || !n_rays || (capacity > 0 && (!origin || !dir))) { set_error("bad argument"); return DR_ERR_INVALID; }
  if (!c->wide || traversal_of(c) != DR_TRAVERSAL_WIDE || !uses_persistent(c)) { set_error("the ray log needs the wide walk and the persistent kernel"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  DR_TRY(join_pipeline(c));      // ordered behind the frames submitted before
  std::vector<float> packed;
  DR_TRY(log_frame_rays(c, settings13, W, H, background, frame_seed, 0x7fffffffull, packed));
  const size_t n = packed.size() / 8;
  *n_rays = n;
  for (size_t i = 0; i < n && i < capacity; i++) { memcpy(origin + 3 * i, &packed[8 * i], 12); memcpy(dir + 3 * i, &packed[8 * i + 4], 12); }
  return DR_OK;
}

}  // extern "C"

// ---- known-answer hooks: n items in, one small kernel, n items out (the common contract: include/dogeray_amd.h "known-answer hooks")
namespace {

// The staging of one hook call: device copies of the caller's inputs, device buffers for its outputs, the launch and the way back.  A failed step is
// remembered and makes every later one a no-op, the launch included.  The buffers live until the call returns.
struct KatStage {
  // !c or n < 0: "bad argument"; then the device; n == 0 is DR_OK before any pointer is looked at (KAT_BEGIN returns it); a null pointer among
  // `required`: "null argument"; needs_scene without one: "no scene uploaded"
  int begin(dr_context* ctx, long long n, std::initializer_list<const void*> required, bool needs_scene) {
    if (!ctx || n < 0) { set_error("bad argument"); return DR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) return DR_OK;
    for (const void* p : required)
      if (!p) { set_error("null argument"); return DR_ERR_INVALID; }
    if (needs_scene && !ctx->walk) { set_error("no scene uploaded"); return DR_ERR_INVALID; }
    c = ctx;
    return DR_OK;
  }
  // a device copy of host[0 .. count)
  template <class T> T* in(const T* host, size_t count) { return static_cast<T*>(stage(host, nullptr, count * sizeof(T), -1)); }
  // a device buffer of count elements that finish() copies to host (null: it stays on the device); preset_byte >= 0: every byte set to it on the stream
  template <class T> T* out(T* host, size_t count, int preset_byte = -1) { return static_cast<T*>(stage(nullptr, host, count * sizeof(T), preset_byte)); }
  // both: a device copy of host[0 .. count) that finish() copies back
  template <class T> T* inout(T* host, size_t count) { return static_cast<T*>(stage(host, host, count * sizeof(T), -1)); }
  // launch(args...) unless a staging step failed -- the in() and out() calls among args have run by now --, then: the launch's error, the stream
  // drained, the outputs in the caller's arrays
  template <class Launch, class... Args> int finish(Launch launch, Args&&... args) {
    DR_TRY(rc);
    launch(std::forward<Args>(args)...);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (const Buf& b : bufs)
      if (b.host) HIP_TRY(hipMemcpy(b.host, b.dev.p, b.bytes, hipMemcpyDeviceToHost));
    return DR_OK;
  }

 private:
  struct Buf { DevMem<unsigned char> dev; void* host = nullptr; size_t bytes = 0; };      // (an allocation each: 256-byte aligned, whatever the element)
  void* stage(const void* src, void* dst, size_t bytes, int preset_byte) {
    if (rc == DR_OK) rc = stage_step(src, dst, bytes, preset_byte);
    return rc == DR_OK ? bufs.back().dev.p : nullptr;
  }
  int stage_step(const void* src, void* dst, size_t bytes, int preset_byte) {
    bufs.emplace_back();
    Buf& b = bufs.back();
    b.host = dst; b.bytes = bytes;
    DR_TRY(b.dev.alloc(bytes));
    if (src) HIP_TRY(hipMemcpy(b.dev.p, src, bytes, hipMemcpyHostToDevice));
    if (preset_byte >= 0) HIP_TRY(hipMemsetAsync(b.dev.p, preset_byte, bytes, c->stream));
    return DR_OK;
  }
  dr_context* c = nullptr;
  std::deque<Buf> bufs;
  int rc = DR_OK;
};

#define KAT_BEGIN(k, c, n, needs_scene, ...) \
  KatStage k;                                \
  if (const int rc_ = k.begin(c, n, {__VA_ARGS__}, needs_scene); rc_ != DR_OK || (n) == 0) return rc_

// slots[i] = the slot of the resident scene that holds object object_index[i] of the file (the inverse of slot_to_orig)
int kat_slots(const dr_context* c, const int32_t* object_index, int n, std::vector<int32_t>& slots) {
  std::vector<int32_t> slot_of((size_t)c->n_prims, -1);
  for (int sidx = 0; sidx < c->n_prims; sidx++) slot_of[(size_t)c->slot_to_orig[(size_t)sidx]] = sidx;
  slots.resize((size_t)n);
  for (int i = 0; i < n; i++) {
    if (object_index[i] < 0 || object_index[i] >= c->n_prims) { set_error("object index out of range"); return DR_ERR_INVALID; }
    slots[(size_t)i] = slot_of[(size_t)object_index[i]];
  }
  return DR_OK;
}

}  // namespace

extern "C" {

int dr_kat_rng(dr_context* c, uint64_t seed, int n, double* out) {
  KAT_BEGIN(k, c, n, false, out);
  DR_TRY(join_pipeline(c));
  return k.finish(launch_kat_rng, c->stream, seed, n, k.out(out, (size_t)n));
}

int dr_kat_aabb(dr_context* c, int n, const float* o, const float* d, const float* mn, const float* mx, int32_t* hit, float* dist) {
  KAT_BEGIN(k, c, n, false, o, d, mn, mx, hit, dist);
  DR_TRY(join_pipeline(c));
  const size_t m = (size_t)n;
  return k.finish(launch_kat_aabb, c->stream, n, k.in(o, 3 * m), k.in(d, 3 * m), k.in(mn, 3 * m), k.in(mx, 3 * m), k.out(hit, m), k.out(dist, m));
}

int dr_kat_node_planes(dr_context* c, int n, const uint32_t* w, const float* a, const float* b, float* t_mix, float* t_cvt) {
  KAT_BEGIN(k, c, n, false, w, a, b, t_mix, t_cvt);
  DR_TRY(join_pipeline(c));
  const size_t m = (size_t)n;
  return k.finish(launch_kat_node_planes, c->stream, n, k.in(w, m), k.in(a, m), k.in(b, m), k.out(t_mix, 4 * m), k.out(t_cvt, 4 * m));
}

int dr_kat_tri(dr_context* c, int n, const float* o, const float* d, const float* v0, const float* v1, const float* v2, float* t) {
  KAT_BEGIN(k, c, n, false, o, d, v0, v1, v2, t);
  DR_TRY(join_pipeline(c));
  const size_t m = (size_t)n;
  return k.finish(launch_kat_tri, c->stream, n, k.in(o, 3 * m), k.in(d, 3 * m), k.in(v0, 3 * m), k.in(v1, 3 * m), k.in(v2, 3 * m), k.out(t, m));
}

int dr_kat_sphere(dr_context* c, int n, const float* o, const float* d, const float* centre, const float* radius, float* t) {
  KAT_BEGIN(k, c, n, false, o, d, centre, radius, t);
  DR_TRY(join_pipeline(c));
  const size_t m = (size_t)n;
  return k.finish(launch_kat_sphere, c->stream, n, k.in(o, 3 * m), k.in(d, 3 * m), k.in(centre, 3 * m), k.in(radius, m), k.out(t, m));
}

int dr_kat_optics(dr_context* c, int n, const float* v, const float* nrm, const float* eta, float* refl, float* refr, float* schlick) {
  KAT_BEGIN(k, c, n, false, v, nrm, eta, refl, refr, schlick);
  DR_TRY(join_pipeline(c));
  const size_t m = (size_t)n;
  return k.finish(launch_kat_optics, c->stream, n, k.in(v, 3 * m), k.in(nrm, 3 * m), k.in(eta, m), k.out(refl, 3 * m), k.out(refr, 3 * m), k.out(schlick, m));
}

int dr_kat_normal(dr_context* c, int n, const int32_t* object_index, const float* o, const float* d, const float* t, float* normal, float* texco) {
  KAT_BEGIN(k, c, n, true, object_index, o, d, t, normal, texco);
  std::vector<int32_t> slots;
  DR_TRY(kat_slots(c, object_index, n, slots));
  DR_TRY(join_pipeline(c));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.prims = c->prims; P.shade = c->shade;
  const size_t m = (size_t)n;
  return k.finish(launch_kat_normal, c->stream, P, n, k.in(slots.data(), m), k.in(o, 3 * m), k.in(d, 3 * m), k.in(t, m), k.out(normal, 3 * m), k.out(texco, 3 * m));
}

// ---- the shading step (device_kat_shade.hpp says what each element writes)
int dr_kat_sample(dr_context* c, int n, const uint64_t* seed, const int32_t* warm, const int32_t* kind, float* point_plain, uint32_t* next_plain,
                  float* point_merged, uint32_t* next_merged) {
  KAT_BEGIN(k, c, n, false, seed, warm, kind, point_plain, next_plain, point_merged, next_merged);
  for (int i = 0; i < n; i++)
    if (warm[i] < 0 || warm[i] > 4096 || (kind[i] != 0 && kind[i] != 2 && kind[i] != 3)) { set_error("warm must be 0 .. 4096, kind 0, 2 or 3"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));
  const size_t m = (size_t)n;
  return k.finish(launch_kat_sample, c->stream, n, k.in(seed, m), k.in(warm, m), k.in(kind, m), k.out(point_plain, 3 * m), k.out(next_plain, 2 * m),
                  k.out(point_merged, 3 * m), k.out(next_merged, 2 * m));
}

int dr_kat_outside(dr_context* c, int n, const float* d2, int32_t* out) {
  KAT_BEGIN(k, c, n, false, d2, out);
  DR_TRY(join_pipeline(c));
  return k.finish(launch_kat_outside, c->stream, n, k.in(d2, (size_t)n), k.out(out, (size_t)n));
}

int dr_kat_tex(dr_context* c, int n, const int32_t* tex, const float* u, const float* v, uint32_t* rgba) {
  KAT_BEGIN(k, c, n, true, tex, u, v, rgba);
  for (int i = 0; i < n; i++)
    if (tex[i] < 0 || tex[i] >= c->n_tex) { set_error("texture index out of range"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.tex = c->tex; P.texels = c->texels;
  const size_t m = (size_t)n;
  return k.finish(launch_kat_tex, c->stream, P, n, k.in(tex, m), k.in(u, m), k.in(v, m), k.out(rgba, m));
}

int dr_kat_bounce(dr_context* c, int n, const int32_t* object_index, const float* o, const float* d, const float* t, const float* atten,
                  const uint64_t* seed, const int32_t* warm, int32_t* alive, float* o_out, float* d_out, float* atten_out, uint32_t* next) {
  KAT_BEGIN(k, c, n, true, object_index, o, d, t, atten, seed, warm, alive, o_out, d_out, atten_out, next);
  std::vector<int32_t> slots;
  DR_TRY(kat_slots(c, object_index, n, slots));
  for (int i = 0; i < n; i++)
    if (warm[i] < 0 || warm[i] > 4096) { set_error("warm must be 0 .. 4096"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.prims = c->prims; P.shade = c->shade; P.tex = c->tex; P.texels = c->texels;
  const size_t m = (size_t)n;
  return k.finish(launch_kat_bounce, c->stream, P, n, k.in(slots.data(), m), k.in(o, 3 * m), k.in(d, 3 * m), k.in(t, m), k.in(atten, 3 * m), k.in(seed, m),
                  k.in(warm, m), k.out(alive, 2 * m), k.out(o_out, 6 * m), k.out(d_out, 6 * m), k.out(atten_out, 6 * m), k.out(next, 4 * m));
}

int dr_kat_miss(dr_context* c, int n, const float* d, const float* atten, int backtex, float background, float* rgb) {
  KAT_BEGIN(k, c, n, true, d, atten, rgb);
  if (backtex >= c->n_tex) { set_error("backtex refers to a texture that is not loaded"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.tex = c->tex; P.texels = c->texels; P.backtex = backtex; P.bgint = background;
  const size_t m = (size_t)n * 3;
  return k.finish(launch_kat_miss, c->stream, P, n, k.in(d, m), k.in(atten, m), k.out(rgb, m));
}

int dr_kat_camera(dr_context* c, const float settings13[13], int W, int H, uint64_t frame_seed, uint32_t seed_stride, int n, const int32_t* x,
                  const int32_t* y, const int32_t* sample, float* origin, float* dir, uint32_t* next) {
  KAT_BEGIN(k, c, n, false, settings13, x, y, sample, origin, dir, next);
  DR_TRY(join_pipeline(c));
  RenderParams P;
  DR_TRY(make_params(c, c->own_site(), settings13, W, H, 0.0f, frame_seed, P, 1));      // the view as a render launch fills it
  P.seed_stride = seed_stride;                                                          // (a launch's is 8 * its block columns)
  const size_t m = (size_t)n;
  return k.finish(launch_kat_camera, c->stream, P, n, k.in(x, m), k.in(y, m), k.in(sample, m), k.out(origin, 6 * m), k.out(dir, 6 * m), k.out(next, 4 * m));
}

int dr_kat_store(dr_context* c, int n, const float* color, int spp, int32_t* out) {
  KAT_BEGIN(k, c, n, false, color, out);
  if (spp < 1) { set_error("null argument, or spp < 1"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));
  const float st[13] = {0, 0, 2, 0, 0, 0, 0, 1, 45, 1, (float)spp, 1, -1};      // any view: the store reads its sample scale alone
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(st, 8, 8, 0.0f, 0, 1, 0, P)) { set_error(why); return DR_ERR_INVALID; }
  const size_t m = (size_t)n * 3;
  P.W = n; P.H = 1; P.out = k.out(out, m); P.accumulate = 0;                   // colour i is pixel (i, 0) of an n x 1 frame
  return k.finish(launch_kat_store, c->stream, P, n, k.in(color, m));
}

int dr_kat_store_merged(dr_context* c, int form, int n_lanes, const int32_t* store_me, const int32_t* key, const int32_t* x, const int32_t* y,
                        const float* color, int spp, int W, int H, int32_t* acc, const int32_t* lds_in, int32_t* lds_out) {
  KAT_BEGIN(k, c, n_lanes, false, store_me, key, x, y, color, acc, lds_in, lds_out);
  if (form < 0 || form > 2) { set_error("store_merged: form must be 0, 1 or 2"); return DR_ERR_INVALID; }
  if (n_lanes % 64 != 0) { set_error("store_merged: n_lanes must be a multiple of 64 (whole waves)"); return DR_ERR_INVALID; }
  if (spp < 1) { set_error("store_merged: spp < 1"); return DR_ERR_INVALID; }
  if (W < 1 || H < 1) { set_error("store_merged: W and H must be at least 1"); return DR_ERR_INVALID; }
  // the kernel adds at (x * H + y) * 3 of acc without a test of its own: every storing lane is judged here
  std::map<int32_t, std::pair<int32_t, int32_t>> pixel_of;
  for (int i = 0; i < n_lanes; i++) {
    if (!store_me[i]) continue;
    if (x[i] < 0 || x[i] >= W || y[i] < 0 || y[i] >= H) { set_error("store_merged: lane " + std::to_string(i) + " stores outside the frame"); return DR_ERR_INVALID; }
    if (key[i] < 0) { set_error("store_merged: lane " + std::to_string(i) + " has a negative key"); return DR_ERR_INVALID; }
    const auto at = pixel_of.emplace(key[i], std::make_pair(x[i], y[i])).first;
    if (at->second != std::make_pair(x[i], y[i])) { set_error("store_merged: lane " + std::to_string(i) + " has the key of another pixel"); return DR_ERR_INVALID; }
  }
  DR_TRY(join_pipeline(c));
  const float st[13] = {0, 0, 2, 0, 0, 0, 0, 1, 45, 1, (float)spp, 1, -1};      // any view, as dr_kat_store: the stores read its sample scale alone
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(st, 8, 8, 0.0f, 0, 1, 0, P)) { set_error(why); return DR_ERR_INVALID; }
  const size_t m = (size_t)n_lanes, words = m / 64 * KAT_MERGE_ROWS * 64;
  P.W = W; P.H = H; P.out = k.inout(acc, (size_t)W * (size_t)H * 3); P.accumulate = 2;
  return k.finish(launch_kat_store_merged, c->stream, P, form, n_lanes, k.in(store_me, m), k.in(key, m), k.in(x, m), k.in(y, m), k.in(color, 3 * m),
                  k.in(lds_in, words), k.out(lds_out, words));
}

int dr_kat_hit(dr_context* c, int n, const float* o, const float* d, float* t, int32_t* idx, int32_t* visits) {
  KAT_BEGIN(k, c, n, true, o, d, t, idx);
  DR_TRY(join_pipeline(c));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  const size_t m = (size_t)n;
  std::vector<int32_t> slots(m);
  DR_TRY(k.finish(launch_kat_hit, c->stream, P, traversal_of(c), n, k.in(o, 3 * m), k.in(d, 3 * m), k.out(t, m), k.out(slots.data(), m),
                  k.out(visits, m)));      // (the kernel counts whether or not the caller asks: visits may be null)
  for (int i = 0; i < n; i++) idx[i] = slots[(size_t)i] >= 0 ? c->slot_to_orig[(size_t)slots[(size_t)i]] : 0;   // hit() returns index 0 on a miss (K:507)
  return DR_OK;
}

int dr_kat_trace(dr_context* c, int variant, int n, const float* o, const float* d, float* t, int32_t* idx) {
  KAT_BEGIN(k, c, n, false, o, d, t, idx);
  if (variant < 0 || variant > 7) { set_error("bad argument"); return DR_ERR_INVALID; }
  if (!c->wide) { set_error("the trace hook needs a resident wide tree (no scene uploaded, or the scene has none)"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));
  // the 8-float layout launch_trace_probe reads: origin, pad, direction, pad
  std::vector<float> packed((size_t)n * 8, 0.0f);
  for (int i = 0; i < n; i++) {
    memcpy(&packed[(size_t)i * 8], o + 3 * (size_t)i, 12);
    memcpy(&packed[(size_t)i * 8 + 4], d + 3 * (size_t)i, 12);
  }
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  std::vector<unsigned> res((size_t)n * 2);      // preset: a ray the kernel did not answer reads as {NaN, -1}, which no walk returns: refused below
  DR_TRY(k.finish(launch_trace_probe, c->stream, P, c->num_cus, variant, k.in(packed.data(), packed.size()), (unsigned)n, k.out<unsigned>(nullptr, 1, 0),
                  k.out(res.data(), res.size(), 0xff)));
  for (int i = 0; i < n; i++) {
    const int32_t slot = (int32_t)res[(size_t)i * 2 + 1];
    if (slot >= c->n_prims) { set_error("the trace kernel returned a slot outside the scene"); return DR_ERR_INVALID; }
    if (slot < 0) {      // {10000, -1}: no hit -- dr_kat_hit's miss; anything else below 0 (the fill above) is a ray the kernel never wrote
      float none = 10000.0f;
      if (slot != -1 || memcmp(&res[(size_t)i * 2], &none, 4) != 0) { set_error("the trace kernel left ray " + std::to_string(i) + " unanswered"); return DR_ERR_DEVICE; }
      t[i] = -1.0f; idx[i] = 0;
    }
    else { memcpy(&t[i], &res[(size_t)i * 2], 4); idx[i] = c->slot_to_orig[(size_t)slot]; }
  }
  return DR_OK;
}

int dr_kat_tile_feedback(dr_context* c, int ntiles, int regions, int heavy_factor, int split_steps, int split_limit, const unsigned* pixel_cost,
                         unsigned* tile_cost, int* order, int* region_start) {
  // what make_params never launches: the order kernel relies on a 64-tile group touching at most two regions
  if (ntiles < 1) { set_error("tile feedback: ntiles must be at least 1"); return DR_ERR_INVALID; }
  if (regions != 1 && regions != MAX_REGIONS) { set_error("tile feedback: regions must be 1 or 8"); return DR_ERR_INVALID; }
  if (regions == MAX_REGIONS && ntiles < 64 * MAX_REGIONS) { set_error("tile feedback: 8 regions need at least 512 tiles (regions of 64 tiles or more)"); return DR_ERR_INVALID; }
  if (split_limit < 0) { set_error("tile feedback: split_limit must not be negative"); return DR_ERR_INVALID; }
  KAT_BEGIN(k, c, ntiles, false, pixel_cost, tile_cost, order, region_start);
  DR_TRY(join_pipeline(c));
  const size_t n = (size_t)ntiles;      // order and region_start preset: an entry the kernels do not write reads as -1
  return k.finish(launch_tile_feedback, c->stream, k.in(pixel_cost, n * 64), k.out(tile_cost, n), k.out(order, n, 0xff),
                  k.out(region_start, (size_t)(2 * MAX_REGIONS + 1), 0xff), ntiles, regions, heavy_factor, split_steps, split_limit);
}

int dr_kat_order_split(dr_context* c, int kind, int ntiles, int regions, const int* order_or_null, const int* region_start, const void* key, int* launch_order,
                       int* launch_region_start, int* dropped_list, unsigned* counts) {
  // the kernel trusts its inputs (it places by them): everything it relies on is judged here
  if (kind != SPLIT_BY_WORD && kind != SPLIT_BY_FLAG) { set_error("order split: kind must be 0 (tile words) or 1 (byte flags)"); return DR_ERR_INVALID; }
  if (ntiles < 1) { set_error("order split: ntiles must be at least 1"); return DR_ERR_INVALID; }
  if (regions < 1 || regions > MAX_REGIONS) { set_error("order split: regions must be 1 .. 8"); return DR_ERR_INVALID; }
  KAT_BEGIN(k, c, ntiles, false, region_start, key, launch_order, launch_region_start, dropped_list, counts);
  bool monotone = region_start[0] == 0 && region_start[regions] == ntiles;
  for (int r = 0; r < regions && monotone; r++) monotone = region_start[r] <= region_start[r + 1];
  if (!monotone) { set_error("order split: region_start must be non-decreasing from 0 to ntiles"); return DR_ERR_INVALID; }
  const size_t n = (size_t)ntiles;
  if (order_or_null) {
    std::vector<bool> seen(n, false);
    for (size_t i = 0; i < n; i++) {
      const int t = order_or_null[i];
      if (t < 0 || t >= ntiles || seen[(size_t)t]) { set_error("order split: order must be a permutation of 0 .. ntiles - 1"); return DR_ERR_INVALID; }
      seen[(size_t)t] = true;
    }
  }
  DR_TRY(join_pipeline(c));
  int own[MAX_REGIONS + 1];      // the identity order's regions travel by value; behind [regions]: ntiles, as make_params leaves them
  for (int r = 0; r <= MAX_REGIONS; r++) own[r] = region_start[r < regions ? r : regions];
  const void* key_dev = kind == SPLIT_BY_WORD ? (const void*)k.in(static_cast<const uint32_t*>(key), n) : (const void*)k.in(static_cast<const uint8_t*>(key), n);
  // every output preset: an entry the kernel does not write reads as -1
  return k.finish(launch_order_split, c->stream, kind, order_or_null ? k.in(order_or_null, n) : nullptr, k.in(region_start, (size_t)(regions + 1)), own, key_dev,
                  ntiles, regions, k.out(launch_order, n, 0xff), k.out(launch_region_start, (size_t)(2 * MAX_REGIONS + 1), 0xff), k.out(dropped_list, n, 0xff),
                  k.out(counts, (size_t)2, 0xff));
}

}  // extern "C"
