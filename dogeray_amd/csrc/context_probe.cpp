// Measurement probes (dr_context_probe_*) and the known-answer hooks of single device functions (dr_kat_*).
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

// ---- KAT hooks
#define KAT_PRE(n)                                                        \
  if (!c || (n) < 0) { set_error("bad argument"); return DR_ERR_INVALID; } \
  HIP_TRY(hipSetDevice(c->device));                                        \
  if ((n) == 0) return DR_OK

int dr_kat_rng(dr_context* c, uint64_t seed, int n, double* out) {
  KAT_PRE(n);
  DevMem<double> d; DR_TRY(d.alloc((size_t)n));
  launch_kat_rng(c->stream, seed, n, d.p);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return d.get(out, (size_t)n);
}

int dr_kat_aabb(dr_context* c, int n, const float* o, const float* d, const float* mn, const float* mx, int32_t* hit, float* dist) {
  KAT_PRE(n);
  DevMem<float> bo, bd, bmn, bmx, bdist; DevMem<int32_t> bhit;
  size_t m = (size_t)n * 3;
  DR_TRY(bo.alloc(m)); DR_TRY(bd.alloc(m)); DR_TRY(bmn.alloc(m)); DR_TRY(bmx.alloc(m)); DR_TRY(bdist.alloc((size_t)n)); DR_TRY(bhit.alloc((size_t)n));
  DR_TRY(bo.put(o, m)); DR_TRY(bd.put(d, m)); DR_TRY(bmn.put(mn, m)); DR_TRY(bmx.put(mx, m));
  launch_kat_aabb(c->stream, n, bo.p, bd.p, bmn.p, bmx.p, bhit.p, bdist.p);
  HIP_TRY(hipStreamSynchronize(c->stream));
  DR_TRY(bhit.get(hit, (size_t)n));
  return bdist.get(dist, (size_t)n);
}

int dr_kat_node_planes(dr_context* c, int n, const uint32_t* w, const float* a, const float* b, float* t_mix, float* t_cvt) {
  KAT_PRE(n);
  DevMem<uint32_t> bw;
  DevMem<float> ba, bb, b1, b2;
  DR_TRY(bw.alloc((size_t)n)); DR_TRY(ba.alloc((size_t)n)); DR_TRY(bb.alloc((size_t)n)); DR_TRY(b1.alloc((size_t)n * 4)); DR_TRY(b2.alloc((size_t)n * 4));
  DR_TRY(bw.put(w, (size_t)n)); DR_TRY(ba.put(a, (size_t)n)); DR_TRY(bb.put(b, (size_t)n));
  launch_kat_node_planes(c->stream, n, bw.p, ba.p, bb.p, b1.p, b2.p);
  HIP_TRY(hipStreamSynchronize(c->stream));
  DR_TRY(b1.get(t_mix, (size_t)n * 4));
  return b2.get(t_cvt, (size_t)n * 4);
}

int dr_kat_tri(dr_context* c, int n, const float* o, const float* d, const float* v0, const float* v1, const float* v2, float* t) {
  KAT_PRE(n);
  DevMem<float> bo, bd, b0, b1, b2, bt;
  size_t m = (size_t)n * 3;
  DR_TRY(bo.alloc(m)); DR_TRY(bd.alloc(m)); DR_TRY(b0.alloc(m)); DR_TRY(b1.alloc(m)); DR_TRY(b2.alloc(m)); DR_TRY(bt.alloc((size_t)n));
  DR_TRY(bo.put(o, m)); DR_TRY(bd.put(d, m)); DR_TRY(b0.put(v0, m)); DR_TRY(b1.put(v1, m)); DR_TRY(b2.put(v2, m));
  launch_kat_tri(c->stream, n, bo.p, bd.p, b0.p, b1.p, b2.p, bt.p);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return bt.get(t, (size_t)n);
}

int dr_kat_sphere(dr_context* c, int n, const float* o, const float* d, const float* centre, const float* radius, float* t) {
  KAT_PRE(n);
  DevMem<float> bo, bd, bc, br, bt;
  size_t m = (size_t)n * 3;
  DR_TRY(bo.alloc(m)); DR_TRY(bd.alloc(m)); DR_TRY(bc.alloc(m)); DR_TRY(br.alloc((size_t)n)); DR_TRY(bt.alloc((size_t)n));
  DR_TRY(bo.put(o, m)); DR_TRY(bd.put(d, m)); DR_TRY(bc.put(centre, m)); DR_TRY(br.put(radius, (size_t)n));
  launch_kat_sphere(c->stream, n, bo.p, bd.p, bc.p, br.p, bt.p);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return bt.get(t, (size_t)n);
}

int dr_kat_optics(dr_context* c, int n, const float* v, const float* nrm, const float* eta, float* refl, float* refr, float* schlick) {
  KAT_PRE(n);
  DevMem<float> bv, bn, be, b1, b2, b3;
  size_t m = (size_t)n * 3;
  DR_TRY(bv.alloc(m)); DR_TRY(bn.alloc(m)); DR_TRY(be.alloc((size_t)n)); DR_TRY(b1.alloc(m)); DR_TRY(b2.alloc(m)); DR_TRY(b3.alloc((size_t)n));
  DR_TRY(bv.put(v, m)); DR_TRY(bn.put(nrm, m)); DR_TRY(be.put(eta, (size_t)n));
  launch_kat_optics(c->stream, n, bv.p, bn.p, be.p, b1.p, b2.p, b3.p);
  HIP_TRY(hipStreamSynchronize(c->stream));
  DR_TRY(b1.get(refl, m)); DR_TRY(b2.get(refr, m));
  return b3.get(schlick, (size_t)n);
}

int dr_kat_normal(dr_context* c, int n, const int32_t* object_index, const float* o, const float* d, const float* t, float* normal, float* texco) {
  KAT_PRE(n);
  if (!c->walk || !object_index || !o || !d || !t || !normal || !texco) { set_error("no scene uploaded, or null argument"); return DR_ERR_INVALID; }
  std::vector<int32_t> slot_of((size_t)c->n_prims, -1), slots((size_t)n);
  for (int sidx = 0; sidx < c->n_prims; sidx++) slot_of[(size_t)c->slot_to_orig[(size_t)sidx]] = sidx;
  for (int i = 0; i < n; i++) {
    if (object_index[i] < 0 || object_index[i] >= c->n_prims) { set_error("object index out of range"); return DR_ERR_INVALID; }
    slots[(size_t)i] = slot_of[(size_t)object_index[i]];
  }
  DevMem<int32_t> bs; DevMem<float> bo, bd, bt, bn, bc;
  size_t m = (size_t)n * 3;
  DR_TRY(bs.alloc((size_t)n)); DR_TRY(bo.alloc(m)); DR_TRY(bd.alloc(m)); DR_TRY(bt.alloc((size_t)n)); DR_TRY(bn.alloc(m)); DR_TRY(bc.alloc(m));
  DR_TRY(bs.put(slots.data(), (size_t)n)); DR_TRY(bo.put(o, m)); DR_TRY(bd.put(d, m)); DR_TRY(bt.put(t, (size_t)n));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.prims = c->prims; P.shade = c->shade;
  launch_kat_normal(c->stream, P, n, bs.p, bo.p, bd.p, bt.p, bn.p, bc.p);
  HIP_TRY(hipStreamSynchronize(c->stream));
  DR_TRY(bn.get(normal, m));
  return bc.get(texco, m);
}

// ---- the shading step (kernels_kat_shade.hip; device_kat_shade.hpp says what each element writes)
int dr_kat_sample(dr_context* c, int n, const uint64_t* seed, const int32_t* warm, const int32_t* kind, float* point_plain, uint32_t* next_plain,
                  float* point_merged, uint32_t* next_merged) {
  KAT_PRE(n);
  if (!seed || !warm || !kind || !point_plain || !next_plain || !point_merged || !next_merged) { set_error("null argument"); return DR_ERR_INVALID; }
  for (int i = 0; i < n; i++)
    if (warm[i] < 0 || warm[i] > 4096 || (kind[i] != 0 && kind[i] != 2 && kind[i] != 3)) { set_error("warm must be 0 .. 4096, kind 0, 2 or 3"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));
  const size_t m = (size_t)n;
  DevMem<uint64_t> bs; DevMem<int32_t> bw, bk; DevMem<float> p1, p2; DevMem<uint32_t> n1, n2;
  DR_TRY(bs.alloc(m)); DR_TRY(bw.alloc(m)); DR_TRY(bk.alloc(m)); DR_TRY(p1.alloc(3 * m)); DR_TRY(p2.alloc(3 * m)); DR_TRY(n1.alloc(2 * m)); DR_TRY(n2.alloc(2 * m));
  DR_TRY(bs.put(seed, m)); DR_TRY(bw.put(warm, m)); DR_TRY(bk.put(kind, m));
  launch_kat_sample(c->stream, n, bs.p, bw.p, bk.p, p1.p, n1.p, p2.p, n2.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  DR_TRY(p1.get(point_plain, 3 * m)); DR_TRY(n1.get(next_plain, 2 * m)); DR_TRY(p2.get(point_merged, 3 * m));
  return n2.get(next_merged, 2 * m);
}

int dr_kat_outside(dr_context* c, int n, const float* d2, int32_t* out) {
  KAT_PRE(n);
  if (!d2 || !out) { set_error("null argument"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));
  DevMem<float> bd; DevMem<int32_t> bo;
  DR_TRY(bd.alloc((size_t)n)); DR_TRY(bo.alloc((size_t)n));
  DR_TRY(bd.put(d2, (size_t)n));
  launch_kat_outside(c->stream, n, bd.p, bo.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  return bo.get(out, (size_t)n);
}

int dr_kat_tex(dr_context* c, int n, const int32_t* tex, const float* u, const float* v, uint32_t* rgba) {
  KAT_PRE(n);
  if (!c->walk || !tex || !u || !v || !rgba) { set_error("no scene uploaded, or null argument"); return DR_ERR_INVALID; }
  for (int i = 0; i < n; i++)
    if (tex[i] < 0 || tex[i] >= c->n_tex) { set_error("texture index out of range"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));
  DevMem<int32_t> bt; DevMem<float> bu, bv; DevMem<uint32_t> bo;
  DR_TRY(bt.alloc((size_t)n)); DR_TRY(bu.alloc((size_t)n)); DR_TRY(bv.alloc((size_t)n)); DR_TRY(bo.alloc((size_t)n));
  DR_TRY(bt.put(tex, (size_t)n)); DR_TRY(bu.put(u, (size_t)n)); DR_TRY(bv.put(v, (size_t)n));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.tex = c->tex; P.texels = c->texels;
  launch_kat_tex(c->stream, P, n, bt.p, bu.p, bv.p, bo.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  return bo.get(rgba, (size_t)n);
}

int dr_kat_bounce(dr_context* c, int n, const int32_t* object_index, const float* o, const float* d, const float* t, const float* atten,
                  const uint64_t* seed, const int32_t* warm, int32_t* alive, float* o_out, float* d_out, float* atten_out, uint32_t* next) {
  KAT_PRE(n);
  if (!c->walk || !object_index || !o || !d || !t || !atten || !seed || !warm || !alive || !o_out || !d_out || !atten_out || !next) {
    set_error("no scene uploaded, or null argument"); return DR_ERR_INVALID;
  }
  std::vector<int32_t> slot_of((size_t)c->n_prims, -1), slots((size_t)n);
  for (int sidx = 0; sidx < c->n_prims; sidx++) slot_of[(size_t)c->slot_to_orig[(size_t)sidx]] = sidx;
  for (int i = 0; i < n; i++) {
    if (object_index[i] < 0 || object_index[i] >= c->n_prims) { set_error("object index out of range"); return DR_ERR_INVALID; }
    if (warm[i] < 0 || warm[i] > 4096) { set_error("warm must be 0 .. 4096"); return DR_ERR_INVALID; }
    slots[(size_t)i] = slot_of[(size_t)object_index[i]];
  }
  DR_TRY(join_pipeline(c));
  const size_t m = (size_t)n;
  DevMem<int32_t> bs, bw, ba; DevMem<float> bo, bd, bt, bat, o2, d2, a2; DevMem<uint64_t> bseed; DevMem<uint32_t> nx;
  DR_TRY(bs.alloc(m)); DR_TRY(bw.alloc(m)); DR_TRY(bo.alloc(3 * m)); DR_TRY(bd.alloc(3 * m)); DR_TRY(bt.alloc(m)); DR_TRY(bat.alloc(3 * m)); DR_TRY(bseed.alloc(m));
  DR_TRY(ba.alloc(2 * m)); DR_TRY(o2.alloc(6 * m)); DR_TRY(d2.alloc(6 * m)); DR_TRY(a2.alloc(6 * m)); DR_TRY(nx.alloc(4 * m));
  DR_TRY(bs.put(slots.data(), m)); DR_TRY(bw.put(warm, m)); DR_TRY(bo.put(o, 3 * m)); DR_TRY(bd.put(d, 3 * m)); DR_TRY(bt.put(t, m)); DR_TRY(bat.put(atten, 3 * m));
  DR_TRY(bseed.put(seed, m));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.prims = c->prims; P.shade = c->shade; P.tex = c->tex; P.texels = c->texels;
  launch_kat_bounce(c->stream, P, n, bs.p, bo.p, bd.p, bt.p, bat.p, bseed.p, bw.p, ba.p, o2.p, d2.p, a2.p, nx.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  DR_TRY(ba.get(alive, 2 * m)); DR_TRY(o2.get(o_out, 6 * m)); DR_TRY(d2.get(d_out, 6 * m)); DR_TRY(a2.get(atten_out, 6 * m));
  return nx.get(next, 4 * m);
}

int dr_kat_miss(dr_context* c, int n, const float* d, const float* atten, int backtex, float background, float* rgb) {
  KAT_PRE(n);
  if (!c->walk || !d || !atten || !rgb) { set_error("no scene uploaded, or null argument"); return DR_ERR_INVALID; }
  if (backtex >= c->n_tex) { set_error("backtex refers to a texture that is not loaded"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));
  const size_t m = (size_t)n * 3;
  DevMem<float> bd, ba, bo;
  DR_TRY(bd.alloc(m)); DR_TRY(ba.alloc(m)); DR_TRY(bo.alloc(m));
  DR_TRY(bd.put(d, m)); DR_TRY(ba.put(atten, m));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.tex = c->tex; P.texels = c->texels; P.backtex = backtex; P.bgint = background;
  launch_kat_miss(c->stream, P, n, bd.p, ba.p, bo.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  return bo.get(rgb, m);
}

int dr_kat_camera(dr_context* c, const float settings13[13], int W, int H, uint64_t frame_seed, uint32_t seed_stride, int n, const int32_t* x,
                  const int32_t* y, const int32_t* sample, float* origin, float* dir, uint32_t* next) {
  KAT_PRE(n);
  if (!settings13 || !x || !y || !sample || !origin || !dir || !next) { set_error("null argument"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));
  RenderParams P;
  DR_TRY(make_params(c, c->own_site(), settings13, W, H, 0.0f, frame_seed, P, 1));      // the view as a render launch fills it
  P.seed_stride = seed_stride;                                                          // (a launch's is 8 * its block columns)
  const size_t m = (size_t)n;
  DevMem<int32_t> bx, by, bs; DevMem<float> bo, bd; DevMem<uint32_t> nx;
  DR_TRY(bx.alloc(m)); DR_TRY(by.alloc(m)); DR_TRY(bs.alloc(m)); DR_TRY(bo.alloc(6 * m)); DR_TRY(bd.alloc(6 * m)); DR_TRY(nx.alloc(4 * m));
  DR_TRY(bx.put(x, m)); DR_TRY(by.put(y, m)); DR_TRY(bs.put(sample, m));
  launch_kat_camera(c->stream, P, n, bx.p, by.p, bs.p, bo.p, bd.p, nx.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  DR_TRY(bo.get(origin, 6 * m)); DR_TRY(bd.get(dir, 6 * m));
  return nx.get(next, 4 * m);
}

int dr_kat_store(dr_context* c, int n, const float* color, int spp, int32_t* out) {
  KAT_PRE(n);
  if (!color || !out || spp < 1) { set_error("null argument, or spp < 1"); return DR_ERR_INVALID; }
  DR_TRY(join_pipeline(c));
  const float st[13] = {0, 0, 2, 0, 0, 0, 0, 1, 45, 1, (float)spp, 1, -1};      // any view: the store reads its sample scale alone
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(st, 8, 8, 0.0f, 0, 1, 0, P)) { set_error(why); return DR_ERR_INVALID; }
  const size_t m = (size_t)n * 3;
  DevMem<float> bc; DevMem<int32_t> bo;
  DR_TRY(bc.alloc(m)); DR_TRY(bo.alloc(m));
  DR_TRY(bc.put(color, m));
  P.W = n; P.H = 1; P.out = bo.p; P.accumulate = 0;                            // colour i is pixel (i, 0) of an n x 1 frame
  launch_kat_store(c->stream, P, n, bc.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  return bo.get(out, m);
}

int dr_kat_hit(dr_context* c, int n, const float* o, const float* d, float* t, int32_t* idx, int32_t* visits) {
  KAT_PRE(n);
  if (!c->walk) { set_error("no scene uploaded"); return DR_ERR_INVALID; }
  DevMem<float> bo, bd, bt; DevMem<int32_t> bs, bv;
  size_t m = (size_t)n * 3;
  DR_TRY(bo.alloc(m)); DR_TRY(bd.alloc(m)); DR_TRY(bt.alloc((size_t)n)); DR_TRY(bs.alloc((size_t)n)); DR_TRY(bv.alloc((size_t)n));
  DR_TRY(bo.put(o, m)); DR_TRY(bd.put(d, m));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  launch_kat_hit(c->stream, P, traversal_of(c), n, bo.p, bd.p, bt.p, bs.p, bv.p);
  HIP_TRY(hipStreamSynchronize(c->stream));
  DR_TRY(bt.get(t, (size_t)n));
  if (visits) DR_TRY(bv.get(visits, (size_t)n));
  std::vector<int32_t> slots((size_t)n);
  DR_TRY(bs.get(slots.data(), (size_t)n));
  for (int i = 0; i < n; i++) idx[i] = slots[(size_t)i] >= 0 ? c->slot_to_orig[(size_t)slots[(size_t)i]] : 0;   // hit() returns index 0 on a miss (K:507)
  return DR_OK;
}

int dr_kat_trace(dr_context* c, int variant, int n, const float* o, const float* d, float* t, int32_t* idx) {
  KAT_PRE(n);
  if (variant < 0 || variant > 7 || !o || !d || !t || !idx) { set_error("bad argument"); return DR_ERR_INVALID; }
  if (!c->wide) { set_error("the trace hook needs a resident wide tree (no scene uploaded, or the scene has none)"); return DR_ERR_INVALID; }
  // the 8-float layout launch_trace_probe reads: origin, pad, direction, pad
  std::vector<float> packed((size_t)n * 8, 0.0f);
  for (int i = 0; i < n; i++) {
    memcpy(&packed[(size_t)i * 8], o + 3 * (size_t)i, 12);
    memcpy(&packed[(size_t)i * 8 + 4], d + 3 * (size_t)i, 12);
  }
  DevMem<float> rays; DevMem<unsigned> cursor, out;
  DR_TRY(rays.alloc((size_t)n * 8)); DR_TRY(cursor.alloc(1)); DR_TRY(out.alloc((size_t)n * 2));
  DR_TRY(rays.put(packed.data(), packed.size()));
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_scene(c, P);
  HIP_TRY(hipMemsetAsync(cursor.p, 0, sizeof(unsigned), c->stream));
  HIP_TRY(hipMemsetAsync(out.p, 0xff, (size_t)n * 2 * sizeof(unsigned), c->stream));      // a ray the kernel did not answer reads as {NaN, -1}, which no walk returns: refused below
  launch_trace_probe(c->stream, P, c->num_cus, variant, rays.p, (unsigned)n, cursor.p, out.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::vector<unsigned> res((size_t)n * 2);
  DR_TRY(out.get(res.data(), res.size()));
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
  if (!c || !pixel_cost || !tile_cost || !order || !region_start) { set_error("null argument"); return DR_ERR_INVALID; }
  // what make_params never launches: the order kernel relies on a 64-tile group touching at most two regions
  if (ntiles < 1) { set_error("tile feedback: ntiles must be at least 1"); return DR_ERR_INVALID; }
  if (regions != 1 && regions != MAX_REGIONS) { set_error("tile feedback: regions must be 1 or 8"); return DR_ERR_INVALID; }
  if (regions == MAX_REGIONS && ntiles < 64 * MAX_REGIONS) { set_error("tile feedback: 8 regions need at least 512 tiles (regions of 64 tiles or more)"); return DR_ERR_INVALID; }
  if (split_limit < 0) { set_error("tile feedback: split_limit must not be negative"); return DR_ERR_INVALID; }
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)ntiles, words = 2 * MAX_REGIONS + 1;
  DevMem<unsigned> bp, bc; DevMem<int> bo, br;
  DR_TRY(bp.alloc(n * 64)); DR_TRY(bc.alloc(n)); DR_TRY(bo.alloc(n)); DR_TRY(br.alloc(words));
  DR_TRY(bp.put(pixel_cost, n * 64));
  HIP_TRY(hipMemsetAsync(bo.p, 0xff, n * sizeof(int), c->stream));             // an entry the kernel does not write reads as -1
  HIP_TRY(hipMemsetAsync(br.p, 0xff, words * sizeof(int), c->stream));
  launch_tile_feedback(c->stream, bp.p, bc.p, bo.p, br.p, ntiles, regions, heavy_factor, split_steps, split_limit);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(c->stream));
  DR_TRY(bc.get(tile_cost, n)); DR_TRY(bo.get(order, n));
  return br.get(region_start, words);
}

}  // extern "C"
