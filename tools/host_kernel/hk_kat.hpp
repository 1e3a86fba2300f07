// The known-answer hooks of the shading step on the host.  Part of host_kernel.cpp.
extern "C" {
// ---- dr_kat_sample .. dr_kat_store on the host: the same per-element bodies (device_kat_shade.hpp) in a loop, the same arguments and layouts
// (include/dogeray_amd.h), the scene's records out of the image of wide_tree = 1.  Each returns 0, or -1 with hk_last_error.
int hk_kat_sample(long long n, const uint64_t* seed, const int32_t* warm, const int32_t* kind, float* point_plain, uint32_t* next_plain, float* point_merged,
                  uint32_t* next_merged) {
  for (long long i = 0; i < n; i++) {
    if (warm[i] < 0 || warm[i] > 4096 || (kind[i] != 0 && kind[i] != 2 && kind[i] != 3)) { hk_err = "warm must be 0 .. 4096, kind 0, 2 or 3"; return -1; }
    kat_sample_lane((int)i, seed, warm, kind, point_plain, next_plain, point_merged, next_merged);
  }
  return 0;
}
int hk_kat_outside(long long n, const float* d2, int32_t* out) {
  for (long long i = 0; i < n; i++) kat_outside_lane((int)i, d2, out);
  return 0;
}
int hk_kat_tex(void* hv, long long n, const int32_t* tex, const float* u, const float* v, uint32_t* rgba) {
  HkScene* h = (HkScene*)hv;
  if (!h) { hk_err = "bad argument"; return -1; }
  const RenderParams P = image_params(h->img);
  for (long long i = 0; i < n; i++) {
    if (tex[i] < 0 || tex[i] >= (int)h->img.tex.size()) { hk_err = "texture index out of range"; return -1; }
    kat_tex_lane(P, (int)i, tex, u, v, rgba);
  }
  return 0;
}
int hk_kat_bounce(void* hv, long long n, const int32_t* object_index, const float* o, const float* d, const float* t, const float* atten, const uint64_t* seed,
                  const int32_t* warm, int32_t* alive, float* o_out, float* d_out, float* atten_out, uint32_t* next) {
  HkScene* h = (HkScene*)hv;
  if (!h || n > 0x7fffffff) { hk_err = "bad argument"; return -1; }
  const DeviceImage& img = h->img;
  const int n_prims = (int)img.slot_to_orig.size();
  std::vector<int32_t> slot_of((size_t)n_prims, -1), slots((size_t)n);
  for (int s = 0; s < n_prims; s++) slot_of[(size_t)img.slot_to_orig[(size_t)s]] = s;
  for (long long i = 0; i < n; i++) {
    if (object_index[i] < 0 || object_index[i] >= n_prims || warm[i] < 0 || warm[i] > 4096) { hk_err = "object index or warm out of range"; return -1; }
    slots[(size_t)i] = slot_of[(size_t)object_index[i]];
  }
  const RenderParams P = image_params(img);
  for (long long i = 0; i < n; i++) kat_bounce_lane(P, (int)i, slots.data(), o, d, t, atten, seed, warm, alive, o_out, d_out, atten_out, next, (int)n);
  return 0;
}
int hk_kat_miss(void* hv, long long n, const float* d, const float* atten, int backtex, float background, float* rgb) {
  HkScene* h = (HkScene*)hv;
  if (!h || backtex >= (int)h->img.tex.size()) { hk_err = "bad argument, or backtex refers to a texture that is not loaded"; return -1; }
  RenderParams P = image_params(h->img);
  P.backtex = backtex; P.bgint = background;
  for (long long i = 0; i < n; i++) kat_miss_lane(P, (int)i, d, atten, rgb);
  return 0;
}
int hk_kat_camera(const float* settings13, int W, int H, uint64_t frame_seed, uint32_t seed_stride, long long n, const int32_t* x, const int32_t* y,
                  const int32_t* sample, float* origin, float* dir, uint32_t* next) {
  RenderParams P;
  if (const char* why = host_view(settings13, W, H, 0.0f, frame_seed, 1, 0, P)) { hk_err = why; return -1; }      // (what make_params fills the view with)
  P.seed_stride = seed_stride;
  for (long long i = 0; i < n; i++) kat_camera_lane(P, (int)i, x, y, sample, origin, dir, next, (int)n);
  return 0;
}
int hk_kat_store(long long n, const float* color, int spp, int32_t* out) {
  if (spp < 1) { hk_err = "spp < 1"; return -1; }
  const float st[13] = {0, 0, 2, 0, 0, 0, 0, 1, 45, 1, (float)spp, 1, -1};
  RenderParams P;
  if (const char* why = host_view(st, 8, 8, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  P.W = (int)n; P.H = 1; P.out = out; P.accumulate = 0;
  for (long long i = 0; i < n; i++) kat_store_lane(P, (int)i, color);
  return 0;
}
}  // extern "C"
