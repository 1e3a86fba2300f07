// The scene handle of the host build and the one path from it to what an entry's loop needs: the image of a tree, the scene and view fields of a
// RenderParams, a lane stack, the closest-hit functor of a walk, the channel writes of an AovHit, and the thread loops.  Part of host_kernel.cpp.
namespace {
thread_local std::string hk_err;

struct HkScene {
  dr_scene* scene = nullptr;
  DeviceImage img;          // the image of wide_tree = 1: the reference's leaf boxes
  DeviceImage own;          // the product's default image (wide_tree = 2: small triangles with their own bounds), built when an entry asks for it
  bool has_own = false;
  // the image of `tree` (2: `own`, built on first use; else `img`); null with hk_err set when the scene cannot be linearised
  const DeviceImage* image(int tree) {
    if (tree != 2) return &img;
    if (!has_own) {
      if (linearise(scene->host, own, 2) != DR_OK) { hk_err = "scene could not be linearised"; return nullptr; }
      has_own = true;
    }
    return &own;
  }
};

// every scene field of P from an image: the host's fill_scene (context_render.cpp)
void fill_image(const DeviceImage& img, RenderParams& P) {
  P.walk = img.walk.data(); P.walk_bytes = (uint32_t)(img.walk.size() * sizeof(DevUnit)); P.pairs = img.pairs.data(); P.prims = img.prims.data();
  P.shade = img.shade.data(); P.tex = img.tex.data(); P.texels = img.texels.data();
  P.wide = img.wide.empty() ? nullptr : img.wide.data(); P.wide_bytes = (uint32_t)(img.wide.size() * sizeof(DevUnit)); P.wide_pmax = img.wide_pmax; P.wide_mu = img.wide_mu;
}
// a P of zeros but for the scene fields of an image: what an entry without a view walks and shades with
RenderParams image_params(const DeviceImage& img) {
  RenderParams P;
  memset(&P, 0, sizeof(P));
  fill_image(img, P);
  return P;
}
// P zeroed, then a view's fields (params_host.hpp fill_view_params); returns the refusal for hk_err, or null
const char* host_view(const float* st13, int W, int H, float bg, uint64_t seed, int mod, int rem, RenderParams& P) {
  memset(&P, 0, sizeof(P));
  return fill_view_params(st13, W, H, bg, seed, mod, rem, P);
}
// the same for a view whose background may be one of the image's textures
const char* host_view(const DeviceImage& img, const float* st13, int W, int H, float bg, uint64_t seed, int mod, int rem, RenderParams& P) {
  if (const char* why = host_view(st13, W, H, bg, seed, mod, rem, P)) return why;
  return P.backtex >= (int)img.tex.size() ? "backtex refers to a texture that is not loaded" : nullptr;
}

// one lane stack, deep enough for every walk, at each of the 64 lane strides
struct HostStack {
  std::vector<int> words = std::vector<int>((size_t)std::max(WIDE_STACK, ORDERED_STACK) * 64);
  int* data() { return words.data(); }
};

// body(closest) with the closest-hit functor of the walk that `traversal` selects -- the wide walk where the image has a wide tree, the ordered walk,
// else the threaded one (a scene without a wide tree takes the threaded walk for DR_TRAVERSAL_WIDE, as the product does).  Call it outside the
// per-ray loop: the three arms are three instantiations of body, each with its walk inlined.
template <bool COUNT, class F>
inline auto with_closest(const RenderParams& P, int traversal, int* stack, F&& body) {
  if (traversal == DR_TRAVERSAL_WIDE && P.wide) {
    const WalkRsrc wide = wide_rsrc(P);
    return body([&, wide](V3 o, V3 d, Ctr& c) { return closest_hit_wide<COUNT>(wide, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, o, d, c, stack); });
  }
  if (traversal == DR_TRAVERSAL_ORDERED) return body([&](V3 o, V3 d, Ctr& c) { return closest_hit_ordered<COUNT>(P.pairs, P.prims, o, d, c, stack); });
  const WalkRsrc walk = walk_rsrc(P);
  return body([&, walk](V3 o, V3 d, Ctr& c) { return closest_hit_threaded<COUNT>(walk, o, d, c); });
}
// body(trace) with trace_ray<WALK, true, ANY> (device_trace.hpp) of the walk a plan chose
template <bool ANY, class F>
inline void with_trace(const RenderParams& P, int walk, int* stack, F&& body) {
  if (walk == DR_TRAVERSAL_WIDE) body([&](V3 o, V3 d, float cap, Ctr& c) { return trace_ray<DR_TRAVERSAL_WIDE, true, ANY>(P, o, d, cap, c, stack); });
  else if (walk == DR_TRAVERSAL_ORDERED) body([&](V3 o, V3 d, float cap, Ctr& c) { return trace_ray<DR_TRAVERSAL_ORDERED, true, ANY>(P, o, d, cap, c, stack); });
  else body([&](V3 o, V3 d, float cap, Ctr& c) { return trace_ray<DR_TRAVERSAL_THREADED, true, ANY>(P, o, d, cap, c, stack); });
}

void st3(float* p, V3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
// the surface channels of a hit at index i (null: not written), as dr_trace_rays and dr_render_aov write them
void write_aov_channels(const AovHit& a, size_t i, int32_t* material, float* distance, float* normal, float* uv, float* albedo) {
  if (material) material[i] = a.mat;
  if (distance) distance[i] = a.distance;
  if (normal) st3(normal + 3 * i, a.normal);
  if (uv) { uv[2 * i] = a.u; uv[2 * i + 1] = a.v; }
  if (albedo) st3(albedo + 3 * i, a.albedo);
}

// f(row) for every row, rows interleaved over the threads (fewer than one: one)
void host_rows(int nthreads, int count, const std::function<void(int)>& f) {
  if (nthreads < 1) nthreads = 1;
  std::vector<std::thread> th;
  for (int k = 0; k < nthreads; k++) th.emplace_back([&, k] { for (int r = k; r < count; r += nthreads) f(r); });
  for (std::thread& t : th) t.join();
}
// f(x, y) for every pixel of a w x h grid
template <class F>
void host_grid(int nthreads, int w, int h, const F& f) {
  host_rows(nthreads, h, [&](int y) { for (int x = 0; x < w; x++) f(x, y); });
}
}  // namespace

extern "C" {
const char* hk_last_error() { return hk_err.c_str(); }

void* hk_scene_load(const char* rts_path, const char* texdir) {
  HkScene* h = new HkScene();
  if (dr_scene_load(rts_path, texdir ? texdir : "", &h->scene) != DR_OK || dr_scene_build_bvh(h->scene, 0) != DR_OK) {
    hk_err = dr_last_error();
    if (h->scene) dr_scene_free(h->scene);
    delete h;
    return nullptr;
  }
  try {
    if (linearise(h->scene->host, h->img, 1) != DR_OK) throw std::string(dr_last_error());
  } catch (...) {
    hk_err = "scene could not be linearised";
    dr_scene_free(h->scene);
    delete h;
    return nullptr;
  }
  return h;
}

void hk_scene_free(void* hv) {
  HkScene* h = (HkScene*)hv;
  if (!h) return;
  if (h->scene) dr_scene_free(h->scene);
  delete h;
}
// what dr_context_get_option reports for the image of `tree` (1 / 2, as hk_hit): out3 = wide_depth (0: no wide tree), wide_own_bounds, wide_nodes
int hk_wide_info(void* hv, int tree, int* out3) {
  HkScene* h = (HkScene*)hv;
  if (!h || !out3 || (tree != 1 && tree != 2)) { hk_err = "bad argument"; return -1; }
  const DeviceImage* im = h->image(tree);
  if (!im) return -1;
  const DeviceImage& img = *im;
  out3[0] = img.wide.empty() ? 0 : img.wide_depth; out3[1] = img.wide.empty() ? 0 : img.wide_own_bounds; out3[2] = img.wide.empty() ? 0 : img.wide_nodes;
  return 0;
}

int hk_has_wide(void* hv) { return ((HkScene*)hv)->img.wide.empty() ? 0 : 1; }
int hk_wide_depth(void* hv) { return ((HkScene*)hv)->img.wide.empty() ? 0 : ((HkScene*)hv)->img.wide_depth; }      // nodes on the longest root-to-leaf path of the wide tree
}  // extern "C"
