// north_star's CPU baseline: "a host-C++ compile of the same kernel".  This file compiles the product's OWN device functions
// (dogeray_amd/csrc/device_core.hpp with -DDR_HOST_BUILD: slab, tri_hit, sphere_hit, the wide and the threaded walk, surface_normal,
// shade_hit / shade_miss, Xorwow, camera_ray, render_pixel -- unchanged source, only the buffer loads become bounds-checked memcpys and the
// function qualifiers vanish) together with the product's host ingest (reader, BVH builder, lineariser, wide-walk builder) into
// tools/libhostkernel.so, and renders frames with std::threads over 8-pixel block columns, one "lane" at a time.
//
// The accumulator stages (hk_denoise, hk_upscale, hk_reproject, hk_moments_add, hk_error) are the product's per-pixel bodies as well
// (device_denoise.hpp, device_upscale.hpp, device_reproject.hpp, device_moments.hpp): this file fills the launch structs of device_launch.h with
// host pointers and loops over the pixels; no stage's arithmetic or indexing is written here.  Parameter defaults and ranges are params_host.hpp's.
//
// It is TEST AND BENCH INFRASTRUCTURE: tests/test_host_kernel.py compares its frames with the oracle's pixel for pixel (a check of the
// kernel's arithmetic that needs no GPU) and bench.py reports it as cpu_baseline.kind "same-source" beside the oracle's "port".
// It is not linked into libdogeray_amd.so, which has no CPU path (dr_context_create fails without a GPU).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#define DR_HOST_BUILD 1
#include "../dogeray_amd/csrc/device_core.hpp"
#include "../dogeray_amd/csrc/device_trace.hpp"
#include "../dogeray_amd/csrc/device_allhits.hpp"
#include "../dogeray_amd/csrc/device_kat_shade.hpp"
#include "../dogeray_amd/csrc/device_denoise.hpp"
#include "../dogeray_amd/csrc/device_moments.hpp"
#include "../dogeray_amd/csrc/device_nearest.hpp"
#include "../dogeray_amd/csrc/device_radiance.hpp"
#include "../dogeray_amd/csrc/device_reproject.hpp"
#include "../dogeray_amd/csrc/device_sky.hpp"
#include "../dogeray_amd/csrc/device_upscale.hpp"
#include "../dogeray_amd/csrc/launch_plan.hpp"
#include "../dogeray_amd/csrc/linearise.hpp"
#include "../dogeray_amd/csrc/params_host.hpp"
#include "../dogeray_amd/csrc/scene_host.hpp"

using namespace dr;

namespace {
struct HkScene {
  dr_scene* scene = nullptr;
  DeviceImage img;
  DeviceImage own;          // the product's default image (wide_tree = 2: small triangles with their own bounds), built when a render asks for it
  bool has_own = false;
};
thread_local std::string hk_err;

// plane / ktab (null: none): the grades of the view's grazing certificate, a byte per tile, and the margin's factor per grade -- the camera ray of
// every path of a tile carries its tile's factor, as the lean build's do (kernels_render.hip; there for a pixel's first sample)
template <bool COUNT>
// eplane (null: none): the entry codes of the view's camera rays, a word per tile (hk_camera_entry) -- the camera ray of every path starts its walk there
void render_columns(const RenderParams& P, int traversal, int first, int step, Ctr& total, const uint8_t* plane = nullptr, const float* ktab = nullptr,
                    const int32_t* eplane = nullptr) {
  std::vector<int> stack((size_t)WIDE_STACK * 64 > (size_t)ORDERED_STACK * 64 ? (size_t)WIDE_STACK * 64 : (size_t)ORDERED_STACK * 64);
  Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
  const WalkRsrc walk = walk_rsrc(P), wide = wide_rsrc(P);
  for (int col = first; col < P.ncols; col += step) {
    const int bx = P.stripe_rem + col * P.stripe_mod;
    for (int by = 0; by < P.gy; by++)
      for (int lane = 0; lane < 64; lane++) {                       // lane l of a tile is pixel (l >> 3, l & 7), as in the kernels
        const int x = bx * 8 + (lane >> 3), y = by * 8 + (lane & 7);
        if (traversal == DR_TRAVERSAL_WIDE && P.wide) {
          bool camera = false;
          const float kt = plane ? ktab[plane[(size_t)col * (size_t)P.gy + (size_t)by] & CERT_MAX_LEVELS] : 1.0f;
          const int entry = eplane ? eplane[(size_t)col * (size_t)P.gy + (size_t)by] : 0;
          auto closest = [&](V3 o, V3 d, Ctr& cc) {
            const float k = camera ? kt : 1.0f;
            const int e = camera ? entry : 0;
            camera = false;
            return closest_hit_wide<COUNT>(wide, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, o, d, cc, stack.data(), k, e);
          };
          render_pixel<COUNT>(P, closest, x, y, c, plane || eplane ? &camera : nullptr);
        } else if (traversal == DR_TRAVERSAL_ORDERED) {
          auto closest = [&](V3 o, V3 d, Ctr& cc) { return closest_hit_ordered<COUNT>(P.pairs, P.prims, o, d, cc, stack.data()); };
          render_pixel<COUNT>(P, closest, x, y, c);
        } else {
          auto closest = [&](V3 o, V3 d, Ctr& cc) { return closest_hit_threaded<COUNT>(walk, o, d, cc); };
          render_pixel<COUNT>(P, closest, x, y, c);
        }
      }
  }
  total = c;
}
// f(row) for every row, rows interleaved over the threads
void host_rows(int nthreads, int count, const std::function<void(int)>& f) {
  std::vector<std::thread> th;
  for (int k = 0; k < nthreads; k++) th.emplace_back([&, k] { for (int r = k; r < count; r += nthreads) f(r); });
  for (std::thread& t : th) t.join();
}
// f(x, y) for every pixel of a w x h grid
template <class F>
void host_grid(int nthreads, int w, int h, const F& f) {
  host_rows(nthreads, h, [&](int y) { for (int x = 0; x < w; x++) f(x, y); });
}

// a parameter set handed over as words: a dr_denoise_params, dr_upscale_params or dr_reproject_params
template <class T>
T params_from_words(const int32_t* words) { T p; memcpy(&p, words, sizeof(T)); return p; }

// The low side of hk_denoise and hk_upscale over the L.gw x L.gh pixel grid (L.D, L.acc, L.hist, L.m2 and the AOV planes L.normal, L.depth,
// L.albedo, L.mat set by the caller), stage by stage as denoise_low_side (context_accum.cpp) launches it: the guide prepare, colour stage 0 and
// -- filter -- the variance pre-pass and the L.D.iterations a-trous passes.  The planes live in `planes`; on return L.src is the plane of the
// result, (e, l) after stage 0, (e, var) after the last pass, and L.guide, L.gz are the guides.
struct HostLow {
  std::vector<float> guide, gz, pa, pb;      // float4 (n, z) | depth gradient | colour planes A, B (float4)
};
void host_denoise_low(DnLaunch& L, bool filter, int nthreads, HostLow& planes) {
  const size_t n = (size_t)L.gw * L.gh;
  planes.guide.resize(4 * n); planes.gz.resize(n); planes.pa.resize(4 * n); planes.pb.resize(4 * n);
  L.guide = planes.guide.data(); L.gz = planes.gz.data();
  host_grid(nthreads, L.gw, L.gh, [&](int x, int y) { dn_guide_pixel(L, x, y); });
  L.dst = planes.pa.data();
  host_grid(nthreads, L.gw, L.gh, [&](int x, int y) { dn_colour_pixel(L, x, y); });            // acc -> (e, l) in A
  L.src = planes.pa.data(); L.dst = planes.pb.data();
  if (!filter) return;
  host_grid(nthreads, L.gw, L.gh, [&](int x, int y) { dn_variance_pixel(L, x, y); });          // (e, l) -> (e, var) in B
  L.src = planes.pb.data(); L.dst = planes.pa.data();                                          // the passes: B -> A -> B ...
  for (int it = 0; it < L.D.iterations; it++) {
    host_grid(nthreads, L.gw, L.gh, [&](int x, int y) { dn_pass_pixel(L, 1 << it, x, y); });
    float* const t = const_cast<float*>(L.src);
    L.src = L.dst; L.dst = t;
  }
}

}  // namespace

extern "C" {

// The restated uniform draws of device_rng.hpp (Xorwow::uniform_double, uniform_pm1, outside_unit) against the plain expressions of
// curand_uniform_double (CUDA 11.2 curand_kernel.h) and of kernel.cu K:640-648: n random generator outputs plus the corners; returns mismatches.
long long hk_check_uniform(long long n, unsigned long long seed) {
  long long bad = 0;
  auto one = [&bad](uint32_t x, uint32_t y) {
    const uint64_t z = (uint64_t)x ^ ((uint64_t)y << 21);
    const volatile double u_plain = (double)z * 1.1102230246251565e-16 + 5.5511151231257827e-17;
    const volatile double t = u_plain * 2;
    const float f_plain = (float)(t - 1);
    const uint32_t lo = x ^ (y << 21), hi = y >> 11;
    const double zh = ((bits_double(0x45300000u, hi) - 19342813118337666422669312.0) + bits_double(0x43300000u, lo)) + 0.5;
    const double u_new = zh * 0x1p-53;
    const float f_new = (float)__builtin_fma(zh, 0x1p-52, -1.0);
    if (memcmp((const void*)&u_plain, &u_new, 8) != 0 || memcmp(&f_plain, &f_new, 4) != 0) bad++;
  };
  uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
  auto rnd = [&s]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  for (long long i = 0; i < n; i++) { const uint64_t r = rnd(); one((uint32_t)r, (uint32_t)(r >> 32)); }
  const uint32_t corners[] = {0u, 1u, 2u, 3u, 0x7ffu, 0x800u, 0x801u, 0x3ffu, 0x400u, 0x401u, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xfffffffeu, 0xffffffffu, 0x001fffffu, 0x00200000u, 0xffe00000u, 0xffdfffffu};
  for (uint32_t a : corners) for (uint32_t b : corners) one(a, b);
  // a texel byte over 255 (byte_over_255) against the division
  for (uint32_t b8 = 0; b8 < 256; b8++) { const volatile float num = (float)b8, den = 255.0f; const float plain = num / den, fast = byte_over_255(b8); if (memcmp(&plain, &fast, 4) != 0) bad++; }
  // the rejection test: floats around 1 (every float within 2^-18 of 1) and a sweep
  auto test = [&bad](float d2) {
    const volatile float l = sqrtf(d2);
    const bool plain = l * l >= 1;
    if (plain != outside_unit(d2)) bad++;
  };
  for (int k = -(1 << 18); k <= (1 << 18); k++) { uint32_t b = 0x3f800000u + (uint32_t)k; float f; memcpy(&f, &b, 4); test(f); }
  for (long long i = 0; i < n / 4; i++) { const uint64_t r = rnd(); test((float)(r >> 40) * (3.0f / 16777216.0f)); }
  return bad;
}

// The merged rejection loop (device_rng.hpp rand_points_merged: candidates classified from 32 bits, the accepted one converted exactly from the
// generator's state) against rand_in_unit_sphere / rand_in_unit_disk on n generator states: the same point, bit for bit, and the same state afterwards.
// Returns mismatches; *max_d2_gap (optional) = the largest |d2~ - d2| seen over all candidates, to set beside the bound of the proof (2^-17).
long long hk_check_reject(long long n, unsigned long long seed, double* max_d2_gap) {
  long long bad = 0;
  double gap = 0;
  uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
  auto rnd = [&s]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  for (long long i = 0; i < n; i++) {
    Xorwow a; a.init(rnd());
    const int warm = (int)(rnd() % 7); for (int k = 0; k < warm; k++) a.next();
    for (int kind = 2; kind <= 3; kind++) {
      Xorwow plain = a, merged = a;
      const V3 want = kind == 3 ? rand_in_unit_sphere(plain) : rand_in_unit_disk(plain);
      const V3 got = rand_points_merged<false>(merged, kind);
      if (memcmp(&want, &got, sizeof(V3)) != 0 || memcmp(&plain, &merged, sizeof(Xorwow)) != 0) bad++;
    }
    // the gap between the approximate and the exact squared length of one candidate of each kind
    Xorwow g = a;
    const uint32_t o[6] = {g.next(), g.next(), g.next(), g.next(), g.next(), g.next()};
    const float xs = (float)__builtin_fma(z_plus_half_of(o[0], o[1]), 0x1p-52, -1.0), ys = (float)__builtin_fma(z_plus_half_of(o[2], o[3]), 0x1p-52, -1.0), zs = (float)__builtin_fma(z_plus_half_of(o[4], o[5]), 0x1p-52, -1.0);
    const float xd = (float)(z_plus_half_of(o[0], o[1]) * 0x1p-53) * 2 - 1, yd = (float)(z_plus_half_of(o[2], o[3]) * 0x1p-53) * 2 - 1;
    const float xa = reject_coord(o[0], o[1]), ya = reject_coord(o[2], o[3]), za = reject_coord(o[4], o[5]);
    const double g3 = fabs((double)dot(mk(xs, ys, zs), mk(xs, ys, zs)) - (double)__builtin_fmaf(za, za, __builtin_fmaf(ya, ya, xa * xa)));
    const double g2 = fabs((double)dot(mk(xd, yd, 0), mk(xd, yd, 0)) - (double)__builtin_fmaf(ya, ya, xa * xa));
    if (g3 > gap) gap = g3;
    if (g2 > gap) gap = g2;
  }
  if (max_d2_gap) *max_d2_gap = gap;
  return bad;
}

// device_wide.hpp wide_ray_margin, for the test of its lemma (tests/test_margin_lemma.py): the position margin of n rays for the scene constants (e, l, v)
void hk_ray_margin(long long n, const float* o, const float* d, float e, float l, float v, float* out) {
  for (long long i = 0; i < n; i++) out[i] = wide_ray_margin(mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]), e, l, v);
}
// The camera rays' grazing certificate (device_cert.hpp cert_leaf) of the scene's triangles for one view, as kernels_aux.hip
// cert_mask_kernel builds it, and a check of what it promises against the kernel's own camera rays (camera_ray: camera_prepare, the lens disk,
// camera_finish).  n_samples times: a triangle, a random point X of its padded box (own bounds + 0.01), the pixel X projects to (+-1), a random
// sample seed; a ray that enters that box (slab(), entry > -0.01, as K:484-488) must have |d . (e1 x e2)| >= a_star if the triangle is certified,
// and lie in a flagged tile if it is not.  e_own: triangles with |e1| |e2| above it are skipped (as never entered with their own bounds).
// out[0..7]: rays through certified boxes, of them below a_star (must be 0), rays through flagged boxes, of them in unflagged tiles (must be 0),
// flagged tiles, tiles, triangles flagged, "every tile" set.  Returns 0, or -1 with hk_last_error.
int hk_cert_check(void* hv, const float* settings13, int W, int H, double a_star, float e_own, long long n_samples, uint64_t seed, long long* out, uint32_t* mask_out) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || !out) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(settings13, W, H, 0.0f, 1, 1, 0, P)) { hk_err = why; return -1; }
  CertView cv;
  if (!fill_cert_view(P, a_star, e_own, cv)) { hk_err = "the view gives no certificate"; return -1; }
  const std::vector<DevPrim>& prims = h->img.prims;
  const int tiles = P.ncols * P.gy, nwords = (tiles + 31) / 32;
  std::vector<uint32_t> mask((size_t)nwords + 2, 0u);
  std::vector<int> kind(prims.size(), 0);
  for (size_t i = 0; i < prims.size(); i++) {
    const DevPrim& p = prims[i];
    if (p.type != 2) continue;
    const float e1[3] = {p.e1x, p.e1y, p.e1z}, e2[3] = {p.e2x, p.e2y, p.e2z};
    int rect[4] = {0, -1, 0, -1};
    const int k = cert_leaf(cv, p.v0, e1, e2, rect);
    kind[i] = k;
    if (k == 2) mask[(size_t)nwords] = 1u;
    if (k == 1)
      for (int col = rect[0]; col <= rect[1]; col++)
        for (int r = rect[2]; r <= rect[3]; r++) { const int b = col * cv.gy + r; mask[(size_t)(b >> 5)] |= 1u << (b & 31); }
  }
  long long flagged = 0, flagged_prims = 0;
  for (int b = 0; b < tiles; b++) flagged += (mask[(size_t)nwords] || ((mask[(size_t)(b >> 5)] >> (b & 31)) & 1u)) ? 1 : 0;
  for (int k : kind) flagged_prims += k != 0;
  if (mask_out) memcpy(mask_out, mask.data(), (size_t)(nwords + 2) * sizeof(uint32_t));
  for (int k = 0; k < 8; k++) out[k] = 0;
  out[4] = flagged; out[5] = tiles; out[6] = flagged_prims; out[7] = mask[(size_t)nwords];
  uint64_t st = seed * 0x9E3779B97F4A7C15ull + 1;
  auto rnd = [&st]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st >> 11) * 0x1p-53; };
  std::vector<size_t> tri;
  for (size_t i = 0; i < prims.size(); i++) {
    const DevPrim& p = prims[i];
    const double n1 = std::sqrt((double)p.e1x * p.e1x + (double)p.e1y * p.e1y + (double)p.e1z * p.e1z), n2 = std::sqrt((double)p.e2x * p.e2x + (double)p.e2y * p.e2y + (double)p.e2z * p.e2z);
    if (p.type == 2 && n1 * n2 <= cv.e_own) tri.push_back(i);
  }
  if (tri.empty()) return 0;
  // half the samples from flagged triangles (when there are any), half from all
  std::vector<size_t> flagged_tri;
  for (size_t i : tri) if (kind[i] != 0) flagged_tri.push_back(i);
  for (long long s = 0; s < n_samples; s++) {
    const bool pick_flagged = !flagged_tri.empty() && (s & 1);
    const size_t i = pick_flagged ? flagged_tri[(size_t)(rnd() * (double)flagged_tri.size()) % flagged_tri.size()] : tri[(size_t)(rnd() * (double)tri.size()) % tri.size()];
    const DevPrim& p = prims[i];
    const double v0[3] = {p.v0[0], p.v0[1], p.v0[2]}, e1[3] = {p.e1x, p.e1y, p.e1z}, e2[3] = {p.e2x, p.e2y, p.e2z};
    float mn[3], mx[3];
    double X[3];
    for (int a = 0; a < 3; a++) {
      const double lo = std::min(v0[a], std::min(v0[a] + e1[a], v0[a] + e2[a])) - 0.01, hi = std::max(v0[a], std::max(v0[a] + e1[a], v0[a] + e2[a])) + 0.01;
      mn[a] = (float)lo; mx[a] = (float)hi;
      X[a] = lo + (hi - lo) * rnd();
    }
    // the pixel X projects to through the pinhole
    double rel[3], z = 0;
    for (int a = 0; a < 3; a++) { rel[a] = X[a] - cv.from[a]; z += rel[a] * cv.w[a]; }
    if (!(z > 0)) continue;
    double pl[3];
    for (int a = 0; a < 3; a++) pl[a] = cv.from[a] + rel[a] * (cv.D / z) - cv.llc[a];
    const double nu = cv.du[0] * pl[0] + cv.du[1] * pl[1] + cv.du[2] * pl[2], nv = cv.dv[0] * pl[0] + cv.dv[1] * pl[1] + cv.dv[2] * pl[2];
    const double fx = std::floor(nu * cv.den_w) + (double)((int)(rnd() * 3.0) - 1), fy = std::floor(nv * cv.den_h) + (double)((int)(rnd() * 3.0) - 1);
    if (!(fx >= 0 && fy >= 0 && fx < cv.nx && fy < cv.ny)) continue;
    const int x = (int)fx, y = (int)fy;
    Xorwow rng;
    rng.init(sample_seed(P, x, y, 0, (int)(rnd() * 1000.0)));
    V3 o, d;
    camera_ray(P, x, y, rng, o, d);
    const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    float dist = 0;
    if (!slab(o, inv, mn, mx, dist) || !(dist > -0.01f)) continue;
    if (kind[i] == 0) {
      const double dd[3] = {d.x, d.y, d.z};
      const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
      const double a = std::fabs(dd[0] * nx + dd[1] * ny + dd[2] * nz);
      out[0]++;
      if (!(a >= a_star)) out[1]++;
    } else {
      const int b = (x >> 3) * cv.gy + (y >> 3);
      out[2]++;
      if (!(mask[(size_t)nwords] || ((mask[(size_t)(b >> 5)] >> (b & 31)) & 1u))) out[3]++;
    }
  }
  return 0;
}
// The graded certificate of one view (option cert_levels): the grades of its tiles as kernels_aux.hip builds them -- the same cert_leaf
// against the ladder of cert_factor (params_host.hpp cert_ladder; graded = 0: the single step) -- and hk_cert_check's sampling check per step: a
// camera ray that enters the padded box of a triangle of grade g must have |d . (e1 x e2)| >= the ladder's step g - 1 (g >= 1), and lie in a tile whose
// grade is <= g (g < n_levels).  out[0..3]: rays through boxes of grade >= 1, of them below their step (must be 0), rays through boxes of grade
// < n_levels, of them in tiles of a higher grade (must be 0); out[4] n_levels, out[5] tiles, out[6] "every tile", out[7] base; out[8 + g] tiles of
// grade g, out[16 + g] rays through boxes of grade g (g = 0 .. 7).  plane_out (may be NULL): the grades, a byte per tile.  Returns 0, or -1.
int hk_cert_levels(void* hv, const float* settings13, int W, int H, int cert_factor, int graded, float e_own, long long n_samples, uint64_t seed, long long* out,
                   uint8_t* plane_out) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || !out || cert_factor < 1) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(settings13, W, H, 0.0f, 1, 1, 0, P)) { hk_err = why; return -1; }
  CertView cv;
  if (!fill_cert_view(P, 1e-4 * (double)cert_factor, e_own, cv)) { hk_err = "the view gives no certificate"; return -1; }
  cert_ladder(cert_factor, graded != 0, cv);
  const std::vector<DevPrim>& prims = h->img.prims;
  const int tiles = P.ncols * P.gy, nl = cv.n_levels;
  std::vector<uint8_t> plane((size_t)tiles, (uint8_t)nl);
  std::vector<int> grade(prims.size(), nl);
  bool every = false;
  for (size_t i = 0; i < prims.size(); i++) {
    const DevPrim& p = prims[i];
    if (p.type != 2) continue;
    const float e1[3] = {p.e1x, p.e1y, p.e1z}, e2[3] = {p.e2x, p.e2y, p.e2z};
    int rect[4] = {0, -1, 0, -1};
    int g = nl;
    const int k = cert_leaf(cv, p.v0, e1, e2, rect, &g);
    if (k == 2) { every = true; g = 0; }
    grade[i] = k == 0 ? nl : g;
    if (k == 1)
      for (int col = rect[0]; col <= rect[1]; col++)
        for (int r = rect[2]; r <= rect[3]; r++) { uint8_t& b = plane[(size_t)col * cv.gy + r]; if (g < b) b = (uint8_t)g; }
  }
  if (every) std::fill(plane.begin(), plane.end(), (uint8_t)0);
  if (plane_out) memcpy(plane_out, plane.data(), plane.size());
  for (int k = 0; k < 24; k++) out[k] = 0;
  out[4] = nl; out[5] = tiles; out[6] = every; out[7] = cv.base;
  for (uint8_t b : plane) out[8 + b]++;
  uint64_t st = seed * 0x9E3779B97F4A7C15ull + 1;
  auto rnd = [&st]() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return (double)(st >> 11) * 0x1p-53; };
  std::vector<size_t> tri, low;      // own-bounds triangles; of them the ones that constrain a tile
  for (size_t i = 0; i < prims.size(); i++) {
    const DevPrim& p = prims[i];
    const double n1 = std::sqrt((double)p.e1x * p.e1x + (double)p.e1y * p.e1y + (double)p.e1z * p.e1z), n2 = std::sqrt((double)p.e2x * p.e2x + (double)p.e2y * p.e2y + (double)p.e2z * p.e2z);
    if (p.type == 2 && n1 * n2 <= cv.e_own) { tri.push_back(i); if (grade[i] < nl) low.push_back(i); }
  }
  if (tri.empty()) return 0;
  for (long long s = 0; s < n_samples; s++) {
    const bool pick_low = !low.empty() && (s & 1);
    const size_t i = pick_low ? low[(size_t)(rnd() * (double)low.size()) % low.size()] : tri[(size_t)(rnd() * (double)tri.size()) % tri.size()];
    const DevPrim& p = prims[i];
    const double v0[3] = {p.v0[0], p.v0[1], p.v0[2]}, e1[3] = {p.e1x, p.e1y, p.e1z}, e2[3] = {p.e2x, p.e2y, p.e2z};
    float mn[3], mx[3];
    double X[3];
    for (int a = 0; a < 3; a++) {
      const double lo = std::min(v0[a], std::min(v0[a] + e1[a], v0[a] + e2[a])) - 0.01, hi = std::max(v0[a], std::max(v0[a] + e1[a], v0[a] + e2[a])) + 0.01;
      mn[a] = (float)lo; mx[a] = (float)hi;
      X[a] = lo + (hi - lo) * rnd();
    }
    double rel[3], z = 0;                      // the pixel X projects to through the pinhole
    for (int a = 0; a < 3; a++) { rel[a] = X[a] - cv.from[a]; z += rel[a] * cv.w[a]; }
    if (!(z > 0)) continue;
    double pl[3];
    for (int a = 0; a < 3; a++) pl[a] = cv.from[a] + rel[a] * (cv.D / z) - cv.llc[a];
    const double nu = cv.du[0] * pl[0] + cv.du[1] * pl[1] + cv.du[2] * pl[2], nv = cv.dv[0] * pl[0] + cv.dv[1] * pl[1] + cv.dv[2] * pl[2];
    const double fx = std::floor(nu * cv.den_w) + (double)((int)(rnd() * 3.0) - 1), fy = std::floor(nv * cv.den_h) + (double)((int)(rnd() * 3.0) - 1);
    if (!(fx >= 0 && fy >= 0 && fx < cv.nx && fy < cv.ny)) continue;
    const int x = (int)fx, y = (int)fy;
    Xorwow rng;
    rng.init(sample_seed(P, x, y, 0, (int)(rnd() * 1000.0)));
    V3 o, d;
    camera_ray(P, x, y, rng, o, d);
    const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    float dist = 0;
    if (!slab(o, inv, mn, mx, dist) || !(dist > -0.01f)) continue;
    const int g = grade[i];
    out[16 + g]++;
    if (g >= 1) {
      const double dd[3] = {d.x, d.y, d.z};
      const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
      const double a = std::fabs(dd[0] * nx + dd[1] * ny + dd[2] * nz);
      out[0]++;
      if (!(a >= cv.level_a[g - 1])) out[1]++;
    }
    if (g < nl) {
      out[2]++;
      if (plane[(size_t)(x >> 3) * cv.gy + (size_t)(y >> 3)] > g) out[3]++;
    }
  }
  return 0;
}
// The camera rays' entry table of one view (option camera_entry) over the product's default tree, as kernels_aux.hip builds it -- the same
// entry_leaf over the leaves in depth-first order, the same entry_tile per tile -- for the block columns bx % col_mod == col_rem.  codes_out (may be NULL):
// the entry codes, a word per tile (local column * tile rows + row).  mutant: 0, or one of device_cert.hpp's ENTRY_MUTANTs (a wrong rule on purpose).
// out[0] tiles, out[1] tiles without a leaf (ENTRY_NONE), out[2] tiles at the root, out[3] tiles at a leaf record, out[4] "every tile at the root",
// out[5] leaves, out[8 + d] tiles whose entry lies d records below the root (d = 0 .. 17; ENTRY_NONE not counted).  Returns 0, -1 with hk_last_error,
// or 1 when the view gives no table (fill_cert_view: a degenerate camera, a lens too wide for the focus plane) or the scene has no wide tree.
int hk_camera_entry(void* hv, const float* settings13, int W, int H, int col_mod, int col_rem, int mutant, int32_t* codes_out, long long* out) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || !out || col_mod < 1 || col_rem < 0 || col_rem >= col_mod) { hk_err = "bad argument"; return -1; }
  if (!h->has_own) {
    if (linearise(h->scene->host, h->own, 2) != DR_OK) { hk_err = "scene could not be linearised"; return -1; }
    h->has_own = true;
  }
  const DeviceImage& img = h->own;
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(settings13, W, H, 0.0f, 1, col_mod, col_rem, P)) { hk_err = why; return -1; }
  CertView cv;
  // (the table asks nothing of the certificate's a_star or of the scene's own-bounds E: any valid pair)
  if (img.wide.empty() || !fill_cert_view(P, 40e-4, img.wide_mu.e > 0.0f ? img.wide_mu.e : 1.0f, cv)) return 1;
  const int tiles = P.ncols * P.gy;
  std::vector<uint32_t> mm(2 * (size_t)tiles + 1, 0xffffffffu);
  entry_mutant = mutant;
  for (size_t rank = 0; rank < img.wide_leaf_rec.size(); rank++) {
    const DevUnit* rec = &img.wide[(size_t)img.wide_leaf_rec[rank] * WIDE_UNITS];
    entry_leaf(cv, rec[0].f, rec[1].f, (uint32_t)rank, mm.data(), tiles);
  }
  for (int k = 0; k < 32; k++) out[k] = 0;
  out[0] = tiles; out[4] = mm[2 * (size_t)tiles] == 0u; out[5] = (long long)img.wide_leaf_rec.size();
  for (int t = 0; t < tiles; t++) {
    const int code = entry_tile(img.wide.data(), img.wide_range.data(), mm[2 * (size_t)t], mm[2 * (size_t)t + 1], mm[2 * (size_t)tiles] == 0u);
    if (codes_out) codes_out[t] = code;
    if (code == ENTRY_NONE) { out[1]++; continue; }
    if (code == 0) out[2]++;
    if (code & 1) out[3]++;
    // its depth: down from the root along the records whose ranges hold the entry's
    const uint32_t lo = img.wide_range[2 * (size_t)(code >> 1)], hi = img.wide_range[2 * (size_t)(code >> 1) + 1];
    uint32_t cur = 0u;
    int d = 0;
    while (cur != (uint32_t)(code >> 1) && d < 17) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(&img.wide[(size_t)cur * WIDE_UNITS]);
      uint32_t next = cur;
      for (uint32_t k = 0; k < 4; k++) {
        const uint32_t ch = wide_node_first_child(w) + k;
        if (((wide_node_valid(w) >> k) & 1u) && img.wide_range[2 * (size_t)ch] <= lo && hi <= img.wide_range[2 * (size_t)ch + 1]) next = ch;
      }
      if (next == cur) break;
      cur = next; d++;
    }
    out[8 + d]++;
  }
  entry_mutant = 0;
  return 0;
}
// What the table promises, by brute force: for every pixel of the stripe and `frames` frames (seeds seed + stride f) the kernel's own camera rays (camera_ray
// with the real sample seeds, settings13's samples per pixel) against EVERY leaf of the default tree -- a leaf whose record's box the ray enters (slab(), the
// reference's test) must lie under the entry of the ray's tile (codes: hk_camera_entry's).  out[0] rays, out[1] (ray, leaf) pairs entered, out[2] of them
// not under the tile's entry (must be 0), out[3] pairs entered in tiles whose entry is below the root.  Returns 0, or -1.
int hk_camera_entry_check(void* hv, const float* settings13, int W, int H, int col_mod, int col_rem, uint64_t seed, uint64_t stride, int frames, int nthreads,
                          const int32_t* codes, long long* out) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || !codes || !out || !h->has_own || h->own.wide.empty() || frames < 1) { hk_err = "bad argument (hk_camera_entry first)"; return -1; }
  const DeviceImage& img = h->own;
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(settings13, W, H, 0.0f, seed, col_mod, col_rem, P)) { hk_err = why; return -1; }
  if (nthreads < 1) nthreads = 1;
  std::vector<long long> part((size_t)nthreads * 4, 0);
  const size_t nleaves = img.wide_leaf_rec.size();
  host_rows(nthreads, P.ncols, [&](int col) {
    long long* acc = &part[(size_t)(col % nthreads) * 4];
    const int bx = P.stripe_rem + col * P.stripe_mod;
    for (int by = 0; by < P.gy; by++) {
      const int code = codes[(size_t)col * (size_t)P.gy + (size_t)by];
      const uint32_t lo = code == ENTRY_NONE ? 1u : img.wide_range[2 * (size_t)(code >> 1)], hi = code == ENTRY_NONE ? 0u : img.wide_range[2 * (size_t)(code >> 1) + 1];
      for (int lane = 0; lane < 64; lane++) {
        const int x = bx * 8 + (lane >> 3), y = by * 8 + (lane & 7);
        for (int f = 0; f < frames; f++)
          for (int s = 0; (float)s < P.spp_f; s++) {
            RenderParams Q = P;
            Q.seed = seed + stride * (uint64_t)f;
            Xorwow rng;
            rng.init(sample_seed(Q, x, y, s));
            V3 o, d;
            camera_ray(Q, x, y, rng, o, d);
            const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
            acc[0]++;
            for (size_t rank = 0; rank < nleaves; rank++) {
              const DevUnit* rec = &img.wide[(size_t)img.wide_leaf_rec[rank] * WIDE_UNITS];
              float dist = 0;
              if (!slab(o, inv, rec[0].f, rec[1].f, dist)) continue;
              acc[1]++;
              if (!(lo <= rank && rank <= hi)) acc[2]++;
              if (code != 0) acc[3]++;
            }
          }
      }
    }
  });
  for (int k = 0; k < 4; k++) { out[k] = 0; for (int t = 0; t < nthreads; t++) out[k] += part[(size_t)t * 4 + k]; }
  return 0;
}
// slab() (device_intersect.hpp: the reference's box test, what hk_camera_entry_check lists leaves with) on n ray / box pairs: 1 entered, 0 not
void hk_slab(long long n, const float* o, const float* d, const float* mn, const float* mx, int32_t* hit) {
  for (long long i = 0; i < n; i++) {
    const V3 dd = mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    float dist = 0;
    hit[i] = slab(mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), mk(1.0f / dd.x, 1.0f / dd.y, 1.0f / dd.z), mn + 3 * i, mx + 3 * i, dist) ? 1 : 0;
  }
}
// the default tree's side arrays and leaf boxes, for the tests: leaves, then per rank the record and its box (mn, mx: 6 floats); range2 (may be NULL): two words per record
long long hk_wide_leaves(void* hv, uint32_t* leaf_rec, float* boxes, uint32_t* range2, long long room_leaves, long long room_records) {
  HkScene* h = (HkScene*)hv;
  if (!h) { hk_err = "bad argument"; return -1; }
  if (!h->has_own) {
    if (linearise(h->scene->host, h->own, 2) != DR_OK) { hk_err = "scene could not be linearised"; return -1; }
    h->has_own = true;
  }
  const DeviceImage& img = h->own;
  const long long n = (long long)img.wide_leaf_rec.size(), nrec = (long long)(img.wide.size() / WIDE_UNITS);
  for (long long r = 0; r < n && r < room_leaves; r++) {
    if (leaf_rec) leaf_rec[r] = img.wide_leaf_rec[(size_t)r];
    if (boxes) { const DevUnit* rec = &img.wide[(size_t)img.wide_leaf_rec[(size_t)r] * WIDE_UNITS]; memcpy(boxes + 6 * r, rec[0].f, 12); memcpy(boxes + 6 * r + 3, rec[1].f, 12); }
  }
  if (range2) memcpy(range2, img.wide_range.data(), (size_t)(nrec < room_records ? nrec : room_records) * 8);
  return n;
}
// the same with the certificate's factor (wide_ray_margin's last argument: 1e-4 / a_star for a certified camera ray, 1 otherwise)
void hk_ray_margin_k(long long n, const float* o, const float* d, float e, float l, float v, float k, float* out) {
  for (long long i = 0; i < n; i++) out[i] = wide_ray_margin(mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]), e, l, v, k);
}
// params_host.hpp cert_factor_k: the factor a certified camera ray carries for a_star
float hk_cert_factor_k(double a_star) { return cert_factor_k(a_star); }
// the scene's WideMu (e, l, v) as the product computes it (wide_tree = 2), for the certificate's own-bounds test (CertView e_own)
int hk_wide_mu(void* hv, float* out3) {
  HkScene* h = (HkScene*)hv;
  if (!h || !out3) { hk_err = "bad argument"; return -1; }
  DeviceImage img;
  if (linearise(h->scene->host, img, 2) != DR_OK) { hk_err = "scene could not be linearised"; return -1; }
  out3[0] = img.wide_mu.e; out3[1] = img.wide_mu.l; out3[2] = img.wide_mu.v;
  return img.wide_own_bounds;
}
// hit_tri (device_intersect.hpp tri_hit) on n ray / triangle pairs: t or -1
void hk_tri_hit(long long n, const float* o, const float* d, const float* v0, const float* e1, const float* e2, float* t) {
  for (long long i = 0; i < n; i++)
    t[i] = tri_hit(mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]), mk(v0[3 * i], v0[3 * i + 1], v0[3 * i + 2]),
                   mk(e1[3 * i], e1[3 * i + 1], e1[3 * i + 2]), mk(e2[3 * i], e2[3 * i + 1], e2[3 * i + 2]));
}

// tri_hit's form that hands out the barycentrics (device_intersect.hpp): t or -1, and uv[2 i], uv[2 i + 1] as the test left them (0 where it never formed them)
void hk_tri_hit_uv(long long n, const float* o, const float* d, const float* v0, const float* e1, const float* e2, float* t, float* uv) {
  for (long long i = 0; i < n; i++) {
    float u = 0.0f, v = 0.0f;
    t[i] = tri_hit(mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]), mk(v0[3 * i], v0[3 * i + 1], v0[3 * i + 2]),
                   mk(e1[3 * i], e1[3 * i + 1], e1[3 * i + 2]), mk(e2[3 * i], e2[3 * i + 1], e2[3 * i + 2]), u, v);
    uv[2 * i] = u; uv[2 * i + 1] = v;
  }
}
// tri_barycentrics (device_surface.hpp: the barycentrics as surface_normal forms them, from the ray's origin) on n ray / triangle pairs
void hk_tri_barycentrics(long long n, const float* o, const float* d, const float* v0, const float* e1, const float* e2, float* uv) {
  for (long long i = 0; i < n; i++) {
    const float4 pA = make_float4(v0[3 * i], v0[3 * i + 1], v0[3 * i + 2], e1[3 * i]), pB = make_float4(e1[3 * i + 1], e1[3 * i + 2], e2[3 * i], e2[3 * i + 1]),
                 pC = make_float4(e2[3 * i + 2], 0.0f, 0.0f, 0.0f);
    tri_barycentrics(pA, pB, pC, ld3(o + 3 * i), ld3(d + 3 * i), uv[2 * i], uv[2 * i + 1]);
  }
}
// What the shade phase forms at n given hits before any draw of a point, one way per call (tests/test_hit_inputs_host.py): form 0 shade_prepare<false>
// (texco: surface_normal's on the same records), form 1 shade_prepare_hit<carried, lazy> (device_shade.hpp: the lean persistent build's).  Hit i: the ray
// (o, d), t, the barycentrics uv (read by the carried forms only), record i of prims (DevPrim) and of shade (DevShade), a generator seeded with seed[i].
// Out: alive (0: the path ended at an emissive surface, `emitted` holds its radiance and sc is untouched), texco[2], sc[16] -- the words of ShadeCtx:
// hitpoint, N, ocolor, add_x, rough, ir, r5, mat, front, 0 --, emitted[3], next[2]: the generator's two following outputs.  Returns 0, or -1 with hk_last_error.
int hk_hit_inputs(long long n, int form, int carried, int lazy, const float* o, const float* d, const float* t, const float* uv, const void* prims, const void* shade,
                  int ntex, const void* tex, const uint32_t* texels, const uint64_t* seed, int32_t* alive, float* texco, uint32_t* sc_words, float* emitted, uint32_t* next) {
  if (n < 0 || n > 0x7fffffff || (form != 0 && form != 1)) { hk_err = "bad argument"; return -1; }
  const DevShade* sh = (const DevShade*)shade;
  for (long long i = 0; i < n; i++)
    if (sh[i].texnum >= ntex || sh[i].rtexnum >= ntex) { hk_err = "a shade record names a texture that is not given"; return -1; }
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.prims = (const DevPrim*)prims; P.shade = sh; P.tex = (const DevTex*)tex; P.texels = texels;
  for (long long i = 0; i < n; i++) {
    Path path; path.rayo = ld3(o + 3 * i); path.raydir = ld3(d + 3 * i); path.atten = mk(0.5f, 0.75f, 1.0f);
    Xorwow rng; rng.init(seed[i]);
    Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
    ShadeCtx sc; memset(&sc, 0, sizeof(sc));
    V3 em = mk(0, 0, 0), tc = mk(0, 0, 0);
    bool on;
    if (form == 0) {
      const float4* pp = reinterpret_cast<const float4*>(P.prims + i);
      const float4* sp = reinterpret_cast<const float4*>(P.shade + i);
      surface_normal(pp[0], pp[1], pp[2], sp[0], sp[1], sp[2], sp[3], sp[4], sp[6], path.rayo, path.raydir, path.rayo + splat(t[i]) * path.raydir, tc);
      on = shade_prepare<false>(P, path, t[i], (int)i, rng, c, sc, em);
    } else {
      const float hu = uv[2 * i], hv = uv[2 * i + 1];
      if (carried && lazy) on = shade_prepare_hit<true, true>(P, path, t[i], (int)i, hu, hv, rng, c, sc, em, &tc);
      else if (carried) on = shade_prepare_hit<true, false>(P, path, t[i], (int)i, hu, hv, rng, c, sc, em, &tc);
      else if (lazy) on = shade_prepare_hit<false, true>(P, path, t[i], (int)i, hu, hv, rng, c, sc, em, &tc);
      else on = shade_prepare_hit<false, false>(P, path, t[i], (int)i, hu, hv, rng, c, sc, em, &tc);
    }
    alive[i] = on ? 1 : 0;
    texco[2 * i] = tc.x; texco[2 * i + 1] = tc.y;
    const float f[13] = {sc.hitpoint.x, sc.hitpoint.y, sc.hitpoint.z, sc.N.x, sc.N.y, sc.N.z, sc.ocolor.x, sc.ocolor.y, sc.ocolor.z, sc.add_x, sc.rough, sc.ir, sc.r5};
    memcpy(sc_words + 16 * i, f, sizeof(f));
    sc_words[16 * i + 13] = (uint32_t)sc.mat; sc_words[16 * i + 14] = sc.front ? 1u : 0u; sc_words[16 * i + 15] = 0u;
    emitted[3 * i] = em.x; emitted[3 * i + 1] = em.y; emitted[3 * i + 2] = em.z;
    next[2 * i] = rng.next(); next[2 * i + 1] = rng.next();
  }
  return 0;
}

// launch_plan.hpp on the host (tests/test_launch_plan_host.py).  cfg6: traversal, occupancy, schedule, num_cus, coop_tiles_per_wave, count;
// out11: the build's eight template arguments (count, occ, trav_min, park_min, unroll, wide, coop, perframe), blocks, log_waves, clear_wave_log
void hk_persistent_plan(const int* cfg6, long long work, int coop_steps, int per_frame, int wave_log_on, int* out11) {
  const PersistentCfg cfg = {cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5] != 0};
  const PersistentPlan p = plan_persistent(cfg, work, coop_steps, per_frame != 0, wave_log_on != 0);
  const PersistentBuild& b = p.build;
  const int v[11] = {b.count, b.occ, b.trav_min, b.park_min, b.unroll, b.wide, b.coop, b.perframe, p.blocks, p.log_waves, p.clear_wave_log};
  memcpy(out11, v, sizeof(v));
}
int hk_persistent_can_store_per_frame(const int* cfg6) { return persistent_can_store_per_frame(PersistentCfg{cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5] != 0}); }
// the instantiations of render_persistent_kernel (DR_PERSISTENT_BUILDS), eight ints each, at most `room` of them; returns how many there are
int hk_persistent_builds(int* out, int room) {
#define HK_BUILD(COUNT, OCC, T, P, U, WIDE, COOP, PERFRAME) {COUNT, OCC, T, P, U, WIDE, COOP, PERFRAME},
  static const int builds[][8] = {DR_PERSISTENT_BUILDS(HK_BUILD)};
#undef HK_BUILD
  const int n = (int)(sizeof(builds) / sizeof(builds[0]));
  if (out && room > 0) memcpy(out, builds, sizeof(builds[0]) * (size_t)(room < n ? room : n));
  return n;
}
int hk_plan_regions(int tiles, int batch_hint, int xcd_regions, int short_one_queue, int tiles_per_wave, int num_cus) {
  return plan_regions(tiles, batch_hint, xcd_regions != 0, short_one_queue != 0, tiles_per_wave, num_cus);
}
// launch_plan.hpp plan_sky_split of the plan hk_persistent_plan returns for the same arguments
int hk_plan_sky_split(const int* cfg6, long long work, int coop_steps, int per_frame, int wave_log_on) {
  const PersistentCfg cfg = {cfg6[0], cfg6[1], cfg6[2], cfg6[3], cfg6[4], cfg6[5] != 0};
  return plan_sky_split(plan_persistent(cfg, work, coop_steps, per_frame != 0, wave_log_on != 0)) ? 1 : 0;
}
// device_sky.hpp sky_split_plain: order may be NULL (identity); launch_region_start 2 * MAX_REGIONS + 1 ints; returns the number of sky tiles
int hk_sky_split(const int* order, const int* region_start, const uint32_t* word, int tiles, int regions, int* launch_order, int* launch_region_start, int* sky_list) {
  return sky_split_plain(order, region_start, word, tiles, regions, launch_order, launch_region_start, sky_list);
}
// device_sky.hpp sky_pixel summed over `frames` frames of a launch (seed, stride: dr_render_accumulate's) for n pixels (xs, ys): out[3 * n].
// Returns 0, or -1 with hk_last_error.
int hk_sky_pixel(void* hv, const float* settings13, int W, int H, float background, uint64_t seed, uint64_t stride, int frames, int n, const int* xs, const int* ys,
                 int32_t* out) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || n < 0 || (n > 0 && (!xs || !ys || !out))) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(settings13, W, H, background, seed, 1, 0, P)) { hk_err = why; return -1; }
  const DeviceImage& img = h->img;
  if (P.backtex >= (int)img.tex.size()) { hk_err = "backtex refers to a texture that is not loaded"; return -1; }
  P.tex = img.tex.data(); P.texels = img.texels.data();
  P.batch = frames; P.batch_seed_stride = stride;
  for (int i = 0; i < n; i++) {
    int r = 0, g = 0, b = 0;
    for (int f = 0; f < frames; f++) {
      int fr, fg, fb;
      sky_pixel(P, xs[i], ys[i], f, fr, fg, fb);
      r += fr; g += fg; b += fb;
    }
    out[3 * i] = r; out[3 * i + 1] = g; out[3 * i + 2] = b;
  }
  return 0;
}
// launch_plan.hpp's sky units (option sky_tiles = 2): how many a launch of `batch` frames with n_sky sky tiles has, and unit u as (position in sky_list,
// first frame, frames)
unsigned hk_sky_units(unsigned n_sky, int batch, int chunk) { return sky_units(n_sky, batch, chunk); }
void hk_sky_unit(unsigned u, int batch, int chunk, int* out3) {
  const SkyUnit s = sky_unit(u, batch, chunk);
  out3[0] = s.index; out3[1] = s.first; out3[2] = s.count;
}
// device_sky.hpp sky_tile_frames, the body the sky kernel and the persistent kernel's retiring waves share, over every unit of a launch of `batch` frames
// (seed, stride: dr_render_accumulate's) whose sky list is sky_list[n_sky], all 64 lanes of each, units in the order `perm` gives (null: ascending): added
// into acc (int32[W * H * 3], P.accumulate = 2) and, cost non-null, the cost words (unsigned[tiles * 64]) written.  Returns the units run, or -1.
long long hk_sky_units_render(void* hv, const float* settings13, int W, int H, float background, uint64_t seed, uint64_t stride, int batch, int chunk, int n_sky,
                              const int* sky_list, const unsigned* perm, int32_t* acc, unsigned* cost) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || batch < 1 || n_sky < 0 || !acc || (n_sky > 0 && !sky_list)) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(settings13, W, H, background, seed, 1, 0, P)) { hk_err = why; return -1; }
  const DeviceImage& img = h->img;
  if (P.backtex >= (int)img.tex.size()) { hk_err = "backtex refers to a texture that is not loaded"; return -1; }
  P.tex = img.tex.data(); P.texels = img.texels.data();
  P.batch = batch; P.batch_seed_stride = stride;
  P.out = acc; P.accumulate = 2;
  P.sky_chunk = sky_chunk_frames(batch, chunk);
  const unsigned n_units = sky_units((unsigned)n_sky, batch, P.sky_chunk);
  for (unsigned k = 0; k < n_units; k++) {
    const SkyUnit s = sky_unit(perm ? perm[k] : k, batch, P.sky_chunk);
    if (s.index < 0 || s.index >= n_sky || sky_list[s.index] < 0 || sky_list[s.index] >= P.ncols * P.gy) { hk_err = "unit outside the list"; return -1; }
    for (int lane = 0; lane < 64; lane++) sky_tile_frames(P, sky_list[s.index], lane, s.first, s.count, cost);
  }
  return (long long)n_units;
}
int hk_plan_split_limit(int num_cus, int occupancy, int split_parts, int split_waves) { return plan_split_limit(num_cus, occupancy, split_parts, split_waves); }

const char* hk_last_error() { return hk_err.c_str(); }

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
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.tex = h->img.tex.data(); P.texels = h->img.texels.data();
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
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.prims = img.prims.data(); P.shade = img.shade.data(); P.tex = img.tex.data(); P.texels = img.texels.data();
  for (long long i = 0; i < n; i++) kat_bounce_lane(P, (int)i, slots.data(), o, d, t, atten, seed, warm, alive, o_out, d_out, atten_out, next, (int)n);
  return 0;
}
int hk_kat_miss(void* hv, long long n, const float* d, const float* atten, int backtex, float background, float* rgb) {
  HkScene* h = (HkScene*)hv;
  if (!h || backtex >= (int)h->img.tex.size()) { hk_err = "bad argument, or backtex refers to a texture that is not loaded"; return -1; }
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.tex = h->img.tex.data(); P.texels = h->img.texels.data(); P.backtex = backtex; P.bgint = background;
  for (long long i = 0; i < n; i++) kat_miss_lane(P, (int)i, d, atten, rgb);
  return 0;
}
int hk_kat_camera(const float* settings13, int W, int H, uint64_t frame_seed, uint32_t seed_stride, long long n, const int32_t* x, const int32_t* y,
                  const int32_t* sample, float* origin, float* dir, uint32_t* next) {
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(settings13, W, H, 0.0f, frame_seed, 1, 0, P)) { hk_err = why; return -1; }      // (what make_params fills the view with)
  P.seed_stride = seed_stride;
  for (long long i = 0; i < n; i++) kat_camera_lane(P, (int)i, x, y, sample, origin, dir, next, (int)n);
  return 0;
}
int hk_kat_store(long long n, const float* color, int spp, int32_t* out) {
  if (spp < 1) { hk_err = "spp < 1"; return -1; }
  const float st[13] = {0, 0, 2, 0, 0, 0, 0, 1, 45, 1, (float)spp, 1, -1};
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(st, 8, 8, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  P.W = (int)n; P.H = 1; P.out = out; P.accumulate = 0;
  for (long long i = 0; i < n; i++) kat_store_lane(P, (int)i, color);
  return 0;
}

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

// dr_kat_hit on the host: the closest hit of n caller rays (o[3n], d[3n]) by the walks of device_core.hpp -- traversal 0 closest_hit_threaded, 1
// closest_hit_ordered, 2 closest_hit_wide<true> over the image of `tree` (1: the reference's leaf boxes; 2: the product's default, small triangles with
// their own bounds, built on first use); a scene without a wide tree takes the threaded walk for traversal 2, as the product does.  Results in
// dr_kat_hit's convention: t (-1: miss), the ORIGINAL object index (0 on a miss), visits (may be NULL): boxes tested.  Returns 0, or -1 with hk_last_error.
int hk_hit(void* hv, int traversal, int tree, long long n, const float* o, const float* d, float* t, int32_t* idx, int32_t* visits) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || (n > 0 && (!o || !d || !t || !idx)) || traversal < 0 || traversal > 2 || (tree != 1 && tree != 2)) { hk_err = "bad argument"; return -1; }
  if (tree == 2 && !h->has_own) {
    if (linearise(h->scene->host, h->own, 2) != DR_OK) { hk_err = "scene could not be linearised"; return -1; }
    h->has_own = true;
  }
  const DeviceImage& img = tree == 2 ? h->own : h->img;
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.walk = img.walk.data(); P.walk_bytes = (uint32_t)(img.walk.size() * sizeof(DevUnit));
  P.wide = img.wide.empty() ? nullptr : img.wide.data(); P.wide_bytes = (uint32_t)(img.wide.size() * sizeof(DevUnit)); P.wide_pmax = img.wide_pmax; P.wide_mu = img.wide_mu;
  P.pairs = img.pairs.data(); P.prims = img.prims.data();
  std::vector<int> stack((size_t)WIDE_STACK * 64 > (size_t)ORDERED_STACK * 64 ? (size_t)WIDE_STACK * 64 : (size_t)ORDERED_STACK * 64);
  const WalkRsrc walk = walk_rsrc(P), wide = wide_rsrc(P);
  for (long long i = 0; i < n; i++) {
    const V3 ro = mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
    Hit hit;
    if (traversal == DR_TRAVERSAL_WIDE && P.wide) hit = closest_hit_wide<true>(wide, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, ro, rd, c, stack.data());
    else if (traversal == DR_TRAVERSAL_ORDERED) hit = closest_hit_ordered<true>(P.pairs, P.prims, ro, rd, c, stack.data());
    else hit = closest_hit_threaded<true>(walk, ro, rd, c);
    t[i] = hit.t;
    idx[i] = hit.slot >= 0 ? img.slot_to_orig[(size_t)hit.slot] : 0;      // hit() returns index 0 on a miss (K:507)
    if (visits) visits[i] = (int32_t)c.V;
  }
  return 0;
}
// dr_trace_rays on the host: the walks of device_trace.hpp (trace_threaded, trace_ordered, trace_wide through trace_ray) on n caller rays, traversal and
// tree as hk_hit's (a scene without a wide tree takes the threaded walk for traversal 2).  mode 0 (DR_TRACE_CLOSEST): t (-1: miss), idx -- the ORIGINAL
// object index, -1 on a miss: dr_trace_rays' `object` --, slot (may be NULL): the hit's slot for hk_ray_surface; mode 1 (DR_TRACE_ANY): occluded 1 / 0.
// tmax NULL: every ray 10000.  visits (may be NULL): boxes tested per ray (the counting build's V).  Returns 0, or -1 with hk_last_error.
int hk_trace(void* hv, int traversal, int tree, int mode, long long n, const float* o, const float* d, const float* tmax, float* t, int32_t* idx,
             int32_t* occluded, int32_t* slot, int32_t* visits) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || traversal < 0 || traversal > 2 || (tree != 1 && tree != 2) || (mode != DR_TRACE_CLOSEST && mode != DR_TRACE_ANY) ||
      (n > 0 && (!o || !d || (mode == DR_TRACE_CLOSEST ? (!t || !idx) : !occluded)))) { hk_err = "bad argument"; return -1; }
  if (tree == 2 && !h->has_own) {
    if (linearise(h->scene->host, h->own, 2) != DR_OK) { hk_err = "scene could not be linearised"; return -1; }
    h->has_own = true;
  }
  const DeviceImage& img = tree == 2 ? h->own : h->img;
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.walk = img.walk.data(); P.walk_bytes = (uint32_t)(img.walk.size() * sizeof(DevUnit));
  P.wide = img.wide.empty() ? nullptr : img.wide.data(); P.wide_bytes = (uint32_t)(img.wide.size() * sizeof(DevUnit)); P.wide_pmax = img.wide_pmax; P.wide_mu = img.wide_mu;
  P.pairs = img.pairs.data(); P.prims = img.prims.data();
  std::vector<int> stack((size_t)WIDE_STACK * 64 > (size_t)ORDERED_STACK * 64 ? (size_t)WIDE_STACK * 64 : (size_t)ORDERED_STACK * 64);
  const int walk = plan_trace(n > 0 ? n : 1, traversal, P.wide != nullptr, 1, QUERY_FORCE_PLAIN).traversal;
  for (long long i = 0; i < n; i++) {
    const V3 ro = mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
    const float cap = tmax ? tmax[i] : 10000.0f;
    Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
    Hit hit;
    if (mode == DR_TRACE_ANY) {
      if (walk == DR_TRAVERSAL_WIDE) hit = trace_ray<DR_TRAVERSAL_WIDE, true, true>(P, ro, rd, cap, c, stack.data());
      else if (walk == DR_TRAVERSAL_ORDERED) hit = trace_ray<DR_TRAVERSAL_ORDERED, true, true>(P, ro, rd, cap, c, stack.data());
      else hit = trace_ray<DR_TRAVERSAL_THREADED, true, true>(P, ro, rd, cap, c, stack.data());
      occluded[i] = hit.slot >= 0 ? 1 : 0;
    } else {
      if (walk == DR_TRAVERSAL_WIDE) hit = trace_ray<DR_TRAVERSAL_WIDE, true, false>(P, ro, rd, cap, c, stack.data());
      else if (walk == DR_TRAVERSAL_ORDERED) hit = trace_ray<DR_TRAVERSAL_ORDERED, true, false>(P, ro, rd, cap, c, stack.data());
      else hit = trace_ray<DR_TRAVERSAL_THREADED, true, false>(P, ro, rd, cap, c, stack.data());
      t[i] = hit.t;
      idx[i] = hit.slot >= 0 ? img.slot_to_orig[(size_t)hit.slot] : -1;
      if (slot) slot[i] = hit.slot;
    }
    if (visits) visits[i] = (int32_t)c.V;
  }
  return 0;
}
// dr_trace_rays' surface pass on the host: device_aov.hpp ray_surface on n rays and their hits (t, slot: hk_trace's, of the same tree); the channels
// (null: not written) as dr_trace_rays writes them.  Returns 0, or -1 with hk_last_error.
int hk_ray_surface(void* hv, int tree, long long n, const float* o, const float* d, const float* t, const int32_t* slot, int32_t* material, float* distance,
                   float* normal, float* uv, float* albedo) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || (tree != 1 && tree != 2) || (n > 0 && (!o || !d || !t || !slot))) { hk_err = "bad argument"; return -1; }
  if (tree == 2 && !h->has_own) {
    if (linearise(h->scene->host, h->own, 2) != DR_OK) { hk_err = "scene could not be linearised"; return -1; }
    h->has_own = true;
  }
  const DeviceImage& img = tree == 2 ? h->own : h->img;
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.prims = img.prims.data(); P.shade = img.shade.data(); P.tex = img.tex.data(); P.texels = img.texels.data();
  for (long long i = 0; i < n; i++) {
    if (slot[i] >= (int32_t)img.prims.size()) { hk_err = "slot outside the scene"; return -1; }
    const AovHit a = ray_surface(P, mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]), t[i], slot[i]);
    if (material) material[i] = a.mat;
    if (distance) distance[i] = a.distance;
    if (normal) { normal[3 * i] = a.normal.x; normal[3 * i + 1] = a.normal.y; normal[3 * i + 2] = a.normal.z; }
    if (uv) { uv[2 * i] = a.u; uv[2 * i + 1] = a.v; }
    if (albedo) { albedo[3 * i] = a.albedo.x; albedo[3 * i + 1] = a.albedo.y; albedo[3 * i + 2] = a.albedo.z; }
  }
  return 0;
}
// launch_plan.hpp plan_trace: out3 = kernel (QUERY_KERNEL_*), the traversal really walked, workgroups
void hk_trace_plan(long long n, int traversal, int has_wide, int num_cus, int force, int* out3) {
  const TracePlan p = plan_trace(n, traversal, has_wide != 0, num_cus, force);
  out3[0] = p.kernel; out3[1] = p.traversal; out3[2] = p.blocks;
}
long long hk_trace_persistent_min_rays() { return TRACE_PERSISTENT_MIN_RAYS; }
// dr_trace_radiance on the host: device_radiance.hpp radiance_ray on n caller rays over the walks of device_core.hpp, traversal and tree as hk_hit's
// (a scene without a wide tree takes the threaded walk for traversal 2).  seed / skip NULL as in dr_radiance_rays; radiance (3n) / bounces (n): NULL not
// written, one of them at least.  The refusals are dr_trace_radiance's.  Returns 0, or -1 with hk_last_error.
int hk_radiance(void* hv, int traversal, int tree, long long n, const float* o, const float* d, const uint64_t* seed, const int32_t* skip, int spp,
                int max_depth, float background, int backtex, uint64_t base_seed, float* radiance, int32_t* bounces) {
  HkScene* h = (HkScene*)hv;
  if (!h || traversal < 0 || traversal > 2 || (tree != 1 && tree != 2)) { hk_err = "bad argument"; return -1; }
  if (n < 0 || n >= (long long)1 << 31) { hk_err = "radiance: the ray count must be in [0, 2^31)"; return -1; }
  if (!o || !d) { hk_err = "radiance: null origin or dir"; return -1; }
  if (!radiance && !bounces) { hk_err = "radiance: no output"; return -1; }
  if (spp < 1 || max_depth < 1) { hk_err = "radiance: spp and max_depth must be >= 1"; return -1; }
  if (backtex >= (int)h->img.tex.size()) { hk_err = "backtex refers to a texture that is not loaded"; return -1; }
  if (skip) for (long long i = 0; i < n; i++) if (skip[i] < 0) { hk_err = "radiance: a skip is negative"; return -1; }
  if (tree == 2 && !h->has_own) {
    if (linearise(h->scene->host, h->own, 2) != DR_OK) { hk_err = "scene could not be linearised"; return -1; }
    h->has_own = true;
  }
  const DeviceImage& img = tree == 2 ? h->own : h->img;
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.walk = img.walk.data(); P.walk_bytes = (uint32_t)(img.walk.size() * sizeof(DevUnit));
  P.wide = img.wide.empty() ? nullptr : img.wide.data(); P.wide_bytes = (uint32_t)(img.wide.size() * sizeof(DevUnit)); P.wide_pmax = img.wide_pmax; P.wide_mu = img.wide_mu;
  P.pairs = img.pairs.data(); P.prims = img.prims.data(); P.shade = img.shade.data(); P.tex = img.tex.data(); P.texels = img.texels.data();
  P.max_depth = max_depth; P.bgint = background; P.backtex = backtex;
  RadianceLaunch R;
  memset(&R, 0, sizeof(R));
  R.origin = o; R.dir = d; R.seed = seed; R.skip = skip; R.n = (unsigned)n; R.spp = spp; R.base_seed = base_seed; R.radiance = radiance; R.bounces = bounces;
  std::vector<int> stack((size_t)WIDE_STACK * 64 > (size_t)ORDERED_STACK * 64 ? (size_t)WIDE_STACK * 64 : (size_t)ORDERED_STACK * 64);
  const int mode = plan_radiance(n > 0 ? n : 1, traversal, P.wide != nullptr, 1, QUERY_FORCE_PLAIN).traversal;
  const WalkRsrc walk = walk_rsrc(P), wide = wide_rsrc(P);
  for (long long i = 0; i < n; i++) {
    if (mode == DR_TRAVERSAL_WIDE) {
      auto closest = [&](V3 ro, V3 rd, Ctr& cc) { return closest_hit_wide<false>(wide, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, ro, rd, cc, stack.data()); };
      radiance_ray(P, R, (unsigned)i, closest);
    } else if (mode == DR_TRAVERSAL_ORDERED) {
      auto closest = [&](V3 ro, V3 rd, Ctr& cc) { return closest_hit_ordered<false>(P.pairs, P.prims, ro, rd, cc, stack.data()); };
      radiance_ray(P, R, (unsigned)i, closest);
    } else {
      auto closest = [&](V3 ro, V3 rd, Ctr& cc) { return closest_hit_threaded<false>(walk, ro, rd, cc); };
      radiance_ray(P, R, (unsigned)i, closest);
    }
  }
  return 0;
}
// dr_query_nearest on the host: the per-query bodies of device_nearest.hpp (nearest_query over nearest_wide or nearest_threaded, then nearest_finish)
// on n points p[3n] with radii rmax (NULL: unbounded).  walk 2: the 4-way records of the image of `tree` (1 / 2, as hk_hit's), 0: the threaded links; a
// scene without a wide tree takes the threaded walk for walk 2, as the product does.  The channels as dr_query_nearest writes them (NULL: not written);
// visits (may be NULL): records visited per query.  Returns 0, or -1 with hk_last_error.
int hk_nearest(void* hv, int walk, int tree, long long n, const float* p, const float* rmax, float* distance, float* d2, int32_t* object, int32_t* material,
               float* point, float* uv, int32_t* visits, int nthreads) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || n >= (long long)1 << 31 || (walk != 0 && walk != 2) || (tree != 1 && tree != 2) || (n > 0 && !p) || nthreads < 1) { hk_err = "bad argument"; return -1; }
  if (tree == 2 && !h->has_own) {
    if (linearise(h->scene->host, h->own, 2) != DR_OK) { hk_err = "scene could not be linearised"; return -1; }
    h->has_own = true;
  }
  const DeviceImage& img = tree == 2 ? h->own : h->img;
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.walk = img.walk.data(); P.walk_bytes = (uint32_t)(img.walk.size() * sizeof(DevUnit));
  P.wide = img.wide.empty() ? nullptr : img.wide.data(); P.wide_bytes = (uint32_t)(img.wide.size() * sizeof(DevUnit));
  P.prims = img.prims.data(); P.shade = img.shade.data();
  std::vector<uint32_t> key(2 * (size_t)n + 2);
  NearestLaunch N;
  memset(&N, 0, sizeof(N));
  N.point = p; N.rmax = rmax; N.n = (unsigned)n; N.lmax = img.near_lmax; N.slot_to_orig = img.slot_to_orig.data(); N.key = key.data();
  N.distance = distance; N.d2 = d2; N.object = object; N.material = material; N.qpoint = point; N.uv = uv;
  const bool wide = plan_nearest(n > 0 ? n : 1, walk == 2 && P.wide != nullptr).wide;
  host_rows(nthreads, nthreads, [&](int k) {
    std::vector<int> stack((size_t)WIDE_STACK * 64);
    for (long long i = k; i < n; i += nthreads) {
      Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
      if (wide) nearest_query<true, true>(P, N, (unsigned)i, c, stack.data());
      else nearest_query<false, true>(P, N, (unsigned)i, c, stack.data());
      if (material || point || uv) nearest_finish(P, N, (unsigned)i);
      if (visits) visits[i] = (int32_t)c.V;
    }
  });
  return 0;
}
// The answer of dr_query_nearest by its definition, with no tree: the minimum of (bits(d2), slot) of nearest_prim over every primitive record of the
// scene, d2 <= fl(rmax rmax).  Channels as hk_nearest's.  The baseline of tools/nearest_rate.py and the reference of tests/test_nearest_host.py.
int hk_nearest_brute(void* hv, long long n, const float* p, const float* rmax, float* distance, float* d2, int32_t* object, int32_t* material, float* point,
                     float* uv, int nthreads) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || (n > 0 && !p) || nthreads < 1) { hk_err = "bad argument"; return -1; }
  const DeviceImage& img = h->img;
  const int np = (int)img.prims.size();
  host_rows(nthreads, nthreads, [&](int k) {
    for (long long i = k; i < n; i += nthreads) {
      const V3 q = mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
      const float r = rmax ? rmax[i] : INFINITY;
      float best = r * r; int slot = -1;
      Nearest bn; bn.q = mk(0, 0, 0); bn.u = bn.v = 0.0f;
      if (r >= 0.0f && std::isfinite(q.x) && std::isfinite(q.y) && std::isfinite(q.z))
        for (int s = 0; s < np; s++) {
          const DevPrim& pr = img.prims[(size_t)s];
          if (pr.type != 0 && pr.type != 2) continue;
          const Nearest a = nearest_prim(pr.type == 0 ? WALK_KIND_SPHERE : WALK_KIND_TRIANGLE, mk(pr.v0[0], pr.v0[1], pr.v0[2]), mk(pr.e1x, pr.e1y, pr.e1z),
                                         mk(pr.e2x, pr.e2y, pr.e2z), q);
          if (!a.cand) continue;
          const uint32_t ka = __float_as_uint(a.d2), kb = __float_as_uint(best);
          if (ka < kb || (ka == kb && slot < 0)) { best = a.d2; slot = s; bn = a; }      // slots ascend: a tie keeps the lower one
        }
      const bool hit = slot >= 0;
      if (!hit) { bn.q = mk(0, 0, 0); bn.u = bn.v = 0.0f; }
      if (d2) d2[i] = hit ? best : 0.0f;
      if (distance) distance[i] = hit ? sqrtf(best) : -1.0f;
      if (object) object[i] = hit ? img.slot_to_orig[(size_t)slot] : -1;
      if (material) material[i] = hit ? img.shade[(size_t)slot].mat : -1;
      if (point) { point[3 * i] = bn.q.x; point[3 * i + 1] = bn.q.y; point[3 * i + 2] = bn.q.z; }
      if (uv) { uv[2 * i] = bn.u; uv[2 * i + 1] = bn.v; }
    }
  });
  return 0;
}
// nearest_prim (device_nearest.hpp) on n point / primitive pairs: kind[n] (WALK_KIND_*), a, b, c[3n] as the records store them -> d2[n] (+inf: never a
// candidate), q[3n], uv[2n]
void hk_nearest_prim(long long n, const int32_t* kind, const float* a, const float* b, const float* c, const float* p, float* d2, float* q, float* uv) {
  for (long long i = 0; i < n; i++) {
    const Nearest r = nearest_prim(kind[i], mk(a[3 * i], a[3 * i + 1], a[3 * i + 2]), mk(b[3 * i], b[3 * i + 1], b[3 * i + 2]), mk(c[3 * i], c[3 * i + 1], c[3 * i + 2]),
                                   mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]));
    d2[i] = r.d2; q[3 * i] = r.q.x; q[3 * i + 1] = r.q.y; q[3 * i + 2] = r.q.z; uv[2 * i] = r.u; uv[2 * i + 1] = r.v;
  }
}
// the scene's primitive records in slot order (both trees share them): kind[n], a, b, c[3n], the original object index and the material; and the
// pruning slack's scene constant.  Returns the number of records (arrays NULL: only that).
long long hk_nearest_prims(void* hv, int32_t* kind, float* a, float* b, float* c, int32_t* orig, int32_t* material, float* lmax) {
  HkScene* h = (HkScene*)hv;
  if (!h) { hk_err = "bad argument"; return -1; }
  const DeviceImage& img = h->img;
  if (lmax) *lmax = img.near_lmax;
  if (kind)
    for (size_t s = 0; s < img.prims.size(); s++) {
      const DevPrim& pr = img.prims[s];
      kind[s] = pr.type == 0 ? WALK_KIND_SPHERE : (pr.type == 2 ? WALK_KIND_TRIANGLE : WALK_KIND_NONE);
      a[3 * s] = pr.v0[0]; a[3 * s + 1] = pr.v0[1]; a[3 * s + 2] = pr.v0[2];
      b[3 * s] = pr.e1x; b[3 * s + 1] = pr.e1y; b[3 * s + 2] = pr.e1z;
      c[3 * s] = pr.e2x; c[3 * s + 1] = pr.e2y; c[3 * s + 2] = pr.e2z;
      orig[s] = img.slot_to_orig[s]; material[s] = img.shade[s].mat;
    }
  return (long long)img.prims.size();
}
int hk_nearest_k() { return NEAREST_K; }
// the records of the walk hk_nearest takes: 4-way records (walk 2, scenes that have them), else the nodes and leaves of the threaded walk
long long hk_nearest_records(void* hv, int walk, int tree) {
  HkScene* h = (HkScene*)hv;
  if (!h) { hk_err = "bad argument"; return -1; }
  if (tree == 2 && !h->has_own) {
    if (linearise(h->scene->host, h->own, 2) != DR_OK) { hk_err = "scene could not be linearised"; return -1; }
    h->has_own = true;
  }
  const DeviceImage& img = tree == 2 ? h->own : h->img;
  if (walk == 2 && !img.wide.empty()) return (long long)(img.wide.size() / WIDE_UNITS);
  return (long long)(2 * img.prims.size() - 1);
}
// dr_trace_all_hits on the host: the per-ray bodies of device_allhits.hpp (allhits_wide or allhits_threaded, allhits_store, allhits_surface) on n caller
// rays with list length max_hits and kind_mask.  walk 2: the 4-way records of the image of `tree` (1 / 2, as hk_hit's), 0: the threaded links; a scene
// without a wide tree takes the threaded walk for walk 2, as the product does.  zero_margin (a switch for tests/test_allhits_host.py): the wide node
// step runs with the ray's margins forced to zero -- fl(o * inv) on both sides --, which the reachability argument does not cover.  The channels as
// dr_trace_all_hits writes them (NULL: not written); visits (may be NULL): records visited per ray.  Returns 0, or -1 with hk_last_error.
int hk_allhits(void* hv, int walk, int tree, long long n, const float* o, const float* d, const float* tmax, int max_hits, int kind_mask, int zero_margin,
               int32_t* count, float* t, int32_t* object, int32_t* material, float* distance, float* normal, float* uv, float* albedo, int32_t* visits, int nthreads) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || n >= (long long)1 << 31 || (walk != 0 && walk != 2) || (tree != 1 && tree != 2) || (n > 0 && (!o || !d)) || nthreads < 1 || max_hits < 0 ||
      max_hits > ALLHITS_MAX || kind_mask <= 0 || kind_mask > 3) { hk_err = "bad argument"; return -1; }
  if (max_hits == 0 && (t || object || material || distance || normal || uv || albedo)) { hk_err = "max_hits 0 returns the count only"; return -1; }
  if (tree == 2 && !h->has_own) {
    if (linearise(h->scene->host, h->own, 2) != DR_OK) { hk_err = "scene could not be linearised"; return -1; }
    h->has_own = true;
  }
  const DeviceImage& img = tree == 2 ? h->own : h->img;
  RenderParams P;
  memset(&P, 0, sizeof(P));
  P.walk = img.walk.data(); P.walk_bytes = (uint32_t)(img.walk.size() * sizeof(DevUnit));
  P.wide = img.wide.empty() ? nullptr : img.wide.data(); P.wide_bytes = (uint32_t)(img.wide.size() * sizeof(DevUnit)); P.wide_pmax = img.wide_pmax; P.wide_mu = img.wide_mu;
  P.prims = img.prims.data(); P.shade = img.shade.data(); P.tex = img.tex.data(); P.texels = img.texels.data();
  const bool wide = plan_allhits(n > 0 ? n : 1, walk == 2 && P.wide != nullptr, 1, QUERY_FORCE_PLAIN).wide;
  const int K = max_hits;
  const bool surface = material || distance || normal || uv || albedo;
  std::vector<uint32_t> hit(surface ? 2 * (size_t)n * (size_t)K : 0);
  const AllHitsSurface S = {distance, material, normal, uv, albedo};
  host_rows(nthreads, nthreads, [&](int k) {
    std::vector<int> stack((size_t)WIDE_STACK * 64);
    std::vector<unsigned> list((size_t)ALLHITS_LIST_WORDS * 64);
    for (long long i = k; i < n; i += nthreads) {
      const V3 ro = mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
      const float tm = tmax ? tmax[i] : 10000.0f;
      Ctr c = {0, 0, 0, 0, 0, 0, 0, 0};
      int cnt = 0;
      if (wide && zero_margin) {
        const float cap = trace_cap(tm);
        if (cap > 0.0f) {
          const V3 inv = mk(1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z);
          WideRay wr = wide_ray(ro, rd, inv, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v);
          wr.on = wr.of = mk(ro.x * wr.inv.x, ro.y * wr.inv.y, ro.z * wr.inv.z);
          allhits_wide<true>(wide_rsrc(P), wr, ro, rd, inv, cap, kind_mask, K, cnt, list.data(), c, stack.data());
        }
      } else if (wide) cnt = allhits_ray<true, true>(P, ro, rd, tm, kind_mask, K, list.data(), c, stack.data());
      else cnt = allhits_ray<false, true>(P, ro, rd, tm, kind_mask, K, list.data(), c, stack.data());
      allhits_store((size_t)i, cnt, K, list.data(), img.slot_to_orig.data(), count, t, object, surface ? hit.data() : nullptr);
      if (surface) for (int e = 0; e < K; e++) allhits_surface(P, o, d, hit.data(), K, (size_t)i * (size_t)K + (size_t)e, S);
      if (visits) visits[i] = (int32_t)c.V;
    }
  });
  return 0;
}
// The answer of dr_trace_all_hits by its definition, with no walk: every leaf record of the pre-order array in storage order (a record's successor is
// known from the record before it: an inner node's hit link, a leaf's next-is-leaf bit), slab() on the record's box, prim_hit_kind on its primitive,
// 0 < t <= cap, the kind mask; the crossings sorted by (bits of t, slot).  count, t, object as hk_allhits'.  The yardstick of tests/test_allhits_host.py.
int hk_allhits_brute(void* hv, long long n, const float* o, const float* d, const float* tmax, int max_hits, int kind_mask, int32_t* count, float* t, int32_t* object,
                     int nthreads) {
  HkScene* h = (HkScene*)hv;
  if (!h || n < 0 || (n > 0 && (!o || !d)) || nthreads < 1 || max_hits < 0 || kind_mask <= 0 || kind_mask > 3) { hk_err = "bad argument"; return -1; }
  const DeviceImage& img = h->img;
  const std::vector<DevUnit>& w = img.walk;
  auto word = [&w](size_t unit, int k) { int32_t v; memcpy(&v, &w[unit].f[k], 4); return v; };
  std::vector<size_t> leaves;
  {
    size_t u = 0;
    bool leaf = false;      // (the root of a scene of two objects or more is an inner node)
    while (u + (leaf ? WALK_UNITS_LEAF : WALK_UNITS_INTERNAL) <= w.size()) {
      if (leaf) {
        leaves.push_back(u);
        const int info = word(u, 3);
        if ((info >> 29) & 1) break;
        leaf = (info >> 28) & 1; u += WALK_UNITS_LEAF;
      } else {
        const int link = word(u, 3);
        if (link < 0) break;
        leaf = link & 1; u += WALK_UNITS_INTERNAL;
      }
    }
  }
  if (leaves.size() != img.prims.size()) { hk_err = "the walk array's leaves do not match the primitives"; return -1; }
  const int K = max_hits;
  host_rows(nthreads, nthreads, [&](int k) {
    std::vector<unsigned long long> keys;
    for (long long i = k; i < n; i += nthreads) {
      const V3 ro = mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]), rd = mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]);
      const float tm = tmax ? tmax[i] : 10000.0f;
      const float cap = tm > 0.0f ? fminf(tm, 10000.0f) : 0.0f;
      keys.clear();
      if (cap > 0.0f) {
        const V3 inv = mk(1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z);
        for (const size_t u : leaves) {
          const float mn[3] = {w[u].f[0], w[u].f[1], w[u].f[2]}, mx[3] = {w[u + 1].f[0], w[u + 1].f[1], w[u + 1].f[2]};
          const int info = word(u, 3), kind = (info >> WALK_SLOT_BITS) & 3, slot = info & ((1 << WALK_SLOT_BITS) - 1);
          if (!((kind == WALK_KIND_TRIANGLE && (kind_mask & 1)) || (kind == WALK_KIND_SPHERE && (kind_mask & 2)))) continue;
          float dist;
          if (!slab(ro, inv, mn, mx, dist)) continue;
          const float th = prim_hit_kind(kind, mk(w[u + 1].f[3], w[u + 2].f[0], w[u + 2].f[1]), mk(w[u + 2].f[2], w[u + 2].f[3], w[u + 3].f[0]),
                                         mk(w[u + 3].f[1], w[u + 3].f[2], w[u + 3].f[3]), ro, rd);
          if (th > 0.0f && th <= cap) keys.push_back(hit_key(th, slot));
        }
        std::sort(keys.begin(), keys.end());
      }
      if (count) count[i] = (int32_t)keys.size();
      for (int e = 0; e < K; e++) {
        const bool have = (size_t)e < keys.size();
        if (t) t[i * K + e] = have ? __uint_as_float((uint32_t)(keys[(size_t)e] >> 32)) : -1.0f;
        if (object) object[i * K + e] = have ? img.slot_to_orig[(size_t)(uint32_t)keys[(size_t)e]] : -1;
      }
    }
  });
  return 0;
}
int hk_allhits_max() { return ALLHITS_MAX; }
int hk_allhits_chunk() { return ALLHITS_CHUNK; }
// launch_plan.hpp plan_allhits: out3 = kernel (QUERY_KERNEL_*), wide (1 / 0), workgroups
void hk_allhits_plan(long long n, int has_wide, int num_cus, int force, int* out3) {
  const AllHitsPlan p = plan_allhits(n, has_wide != 0, num_cus, force);
  out3[0] = p.kernel; out3[1] = p.wide ? 1 : 0; out3[2] = p.blocks;
}
long long hk_allhits_persistent_min_rays() { return ALLHITS_PERSISTENT_MIN_RAYS; }
// launch_plan.hpp plan_radiance: out3 = kernel (QUERY_KERNEL_*), the traversal really walked, workgroups
void hk_radiance_plan(long long n, int traversal, int has_wide, int num_cus, int force, int* out3) {
  const RadiancePlan p = plan_radiance(n, traversal, has_wide != 0, num_cus, force);
  out3[0] = p.kernel; out3[1] = p.traversal; out3[2] = p.blocks;
}
long long hk_radiance_persistent_min_rays() { return RADIANCE_PERSISTENT_MIN_RAYS; }
int hk_radiance_chunk() { return RADIANCE_CHUNK; }
int hk_radiance_occ() { return RADIANCE_OCC; }
int hk_radiance_refill_min() { return RADIANCE_REFILL_MIN; }
int hk_radiance_park() { return RADIANCE_PARK; }
// what dr_context_get_option reports for the image of `tree` (1 / 2, as hk_hit): out3 = wide_depth (0: no wide tree), wide_own_bounds, wide_nodes
int hk_wide_info(void* hv, int tree, int* out3) {
  HkScene* h = (HkScene*)hv;
  if (!h || !out3 || (tree != 1 && tree != 2)) { hk_err = "bad argument"; return -1; }
  if (tree == 2 && !h->has_own) {
    if (linearise(h->scene->host, h->own, 2) != DR_OK) { hk_err = "scene could not be linearised"; return -1; }
    h->has_own = true;
  }
  const DeviceImage& img = tree == 2 ? h->own : h->img;
  out3[0] = img.wide.empty() ? 0 : img.wide_depth; out3[1] = img.wide.empty() ? 0 : img.wide_own_bounds; out3[2] = img.wide.empty() ? 0 : img.wide_nodes;
  return 0;
}

int hk_has_wide(void* hv) { return ((HkScene*)hv)->img.wide.empty() ? 0 : 1; }
int hk_wide_depth(void* hv) { return ((HkScene*)hv)->img.wide.empty() ? 0 : ((HkScene*)hv)->img.wide_depth; }      // nodes on the longest root-to-leaf path of the wide tree

// One frame (dr_render_frame's arguments): int32[W * H * 3], pixel (x, y) at (x * H + y) * 3, unrendered margins 0; only the block
// columns bx % col_mod == col_rem are rendered (a bounded sample for the bench).  counters: rays, V, L, S, T, samples (6 words).
// level_plane (may be NULL): the grades of the view's graded certificate (hk_cert_levels' plane_out for cert_factor / graded, whole frame: col_mod 1) --
// the frame is then rendered as the device renders it: the wide walk over the product's default tree (wide_tree = 2), the camera rays with their
// tile's margin.  entry_plane (may be NULL): the entry codes of the view's camera rays for this very stripe (hk_camera_entry's codes_out): the camera rays
// start there, over the default tree as well.
int hk_render(void* hv, const float* settings13, int W, int H, float background, uint64_t frame_seed, int traversal, int nthreads, int col_mod, int col_rem,
              int32_t* out, uint64_t* counters, const uint8_t* level_plane, int cert_factor, int graded, const int32_t* entry_plane) {
  HkScene* h = (HkScene*)hv;
  if (!h || !settings13 || !out || col_mod < 1 || col_rem < 0 || col_rem >= col_mod) { hk_err = "bad argument"; return -1; }
  float ktab[CERT_MAX_LEVELS + 1];
  for (float& k : ktab) k = 1.0f;
  if (level_plane) {
    if (col_mod != 1 || cert_factor < 1 || traversal != DR_TRAVERSAL_WIDE) { hk_err = "a level plane needs the whole frame, its cert_factor and the wide walk"; return -1; }
  }
  const bool own = level_plane || entry_plane;
  if (own) {
    if (traversal != DR_TRAVERSAL_WIDE) { hk_err = "an entry plane needs the wide walk"; return -1; }
    if (!h->has_own) {
      if (linearise(h->scene->host, h->own, 2) != DR_OK) { hk_err = "scene could not be linearised"; return -1; }
      h->has_own = true;
    }
  }
  if (level_plane) {
    CertView cv;
    cert_ladder(cert_factor, graded != 0, cv);
    for (int g = 1; g <= cv.n_levels; g++) ktab[g] = cert_factor_k(cv.level_a[g - 1]);
  }
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(settings13, W, H, background, frame_seed, col_mod, col_rem, P)) { hk_err = why; return -1; }
  const DeviceImage& img = own ? h->own : h->img;
  if (P.backtex >= (int)img.tex.size()) { hk_err = "backtex refers to a texture that is not loaded"; return -1; }
  if (own && img.wide.empty()) { hk_err = "the scene has no wide tree"; return -1; }
  P.walk = img.walk.data(); P.walk_bytes = (uint32_t)(img.walk.size() * sizeof(DevUnit));
  P.wide = img.wide.empty() ? nullptr : img.wide.data(); P.wide_bytes = (uint32_t)(img.wide.size() * sizeof(DevUnit)); P.wide_pmax = img.wide_pmax; P.wide_mu = img.wide_mu;
  P.pairs = img.pairs.data(); P.prims = img.prims.data(); P.shade = img.shade.data(); P.tex = img.tex.data(); P.texels = img.texels.data();
  P.out = out;
  P.accumulate = 0;
  memset(out, 0, (size_t)W * H * 3 * sizeof(int32_t));
  if (nthreads < 1) nthreads = 1;
  std::vector<Ctr> part((size_t)nthreads);
  std::vector<std::thread> th;
  for (int t = 0; t < nthreads; t++)
    th.emplace_back([&, t] {
      if (counters) render_columns<true>(P, traversal, t, nthreads, part[(size_t)t], level_plane, ktab, entry_plane);
      else render_columns<false>(P, traversal, t, nthreads, part[(size_t)t], level_plane, ktab, entry_plane);
    });
  for (std::thread& t : th) t.join();
  if (counters) {
    for (int k = 0; k < 6; k++) counters[k] = 0;
    for (const Ctr& c : part) { counters[0] += c.rays; counters[1] += c.V; counters[2] += c.L; counters[3] += c.S; counters[4] += c.T; counters[5] += c.samples; }
  }
  return 0;
}

// dr_render_aov on the host: device_aov.hpp aov_first_hit for every pixel of the window (x0, y0, w, h) of the pixel grid, with the given traversal;
// the channels (null: not written) in dr_render_aov's layout.  Returns 0, or -1 with hk_last_error.
int hk_aov(void* hv, const float* settings13, int W, int H, int x0, int y0, int w, int h, int traversal, int nthreads, float* t, float* distance,
           float* depth, int32_t* object, int32_t* material, float* normal, float* uv, float* albedo, float* dir) {
  HkScene* h_ = (HkScene*)hv;
  if (!h_ || !settings13) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(settings13, W, H, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  const DeviceImage& img = h_->img;
  if (P.backtex >= (int)img.tex.size()) { hk_err = "backtex refers to a texture that is not loaded"; return -1; }
  if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || x0 > P.gx * 8 - w || y0 > P.gy * 8 - h) { hk_err = "window is empty or not inside the pixel grid"; return -1; }
  P.walk = img.walk.data(); P.walk_bytes = (uint32_t)(img.walk.size() * sizeof(DevUnit));
  P.wide = img.wide.empty() ? nullptr : img.wide.data(); P.wide_bytes = (uint32_t)(img.wide.size() * sizeof(DevUnit)); P.wide_pmax = img.wide_pmax; P.wide_mu = img.wide_mu;
  P.pairs = img.pairs.data(); P.prims = img.prims.data(); P.shade = img.shade.data(); P.tex = img.tex.data(); P.texels = img.texels.data();
  const float focus = settings13[7];
  if (nthreads < 1) nthreads = 1;
  std::vector<std::thread> th;
  for (int k = 0; k < nthreads; k++)
    th.emplace_back([&, k] {
      std::vector<int> stack((size_t)WIDE_STACK * 64 > (size_t)ORDERED_STACK * 64 ? (size_t)WIDE_STACK * 64 : (size_t)ORDERED_STACK * 64);
      const WalkRsrc walk = walk_rsrc(P), wide = wide_rsrc(P);
      for (int wy = k; wy < h; wy += nthreads)
        for (int wx = 0; wx < w; wx++) {
          AovHit a;
          if (traversal == DR_TRAVERSAL_WIDE && P.wide) {
            auto closest = [&](V3 o, V3 d, Ctr& cc) { return closest_hit_wide<false>(wide, P.wide_pmax, P.wide_mu.e, P.wide_mu.l, P.wide_mu.v, o, d, cc, stack.data()); };
            a = aov_first_hit(P, closest, focus, x0 + wx, y0 + wy);
          } else if (traversal == DR_TRAVERSAL_ORDERED) {
            auto closest = [&](V3 o, V3 d, Ctr& cc) { return closest_hit_ordered<false>(P.pairs, P.prims, o, d, cc, stack.data()); };
            a = aov_first_hit(P, closest, focus, x0 + wx, y0 + wy);
          } else {
            auto closest = [&](V3 o, V3 d, Ctr& cc) { return closest_hit_threaded<false>(walk, o, d, cc); };
            a = aov_first_hit(P, closest, focus, x0 + wx, y0 + wy);
          }
          const size_t i = (size_t)wy * (size_t)w + (size_t)wx;
          if (t) t[i] = a.t;
          if (distance) distance[i] = a.distance;
          if (depth) depth[i] = a.depth;
          if (object) object[i] = a.slot >= 0 ? img.slot_to_orig[(size_t)a.slot] : -1;
          if (material) material[i] = a.mat;
          if (normal) { normal[3 * i] = a.normal.x; normal[3 * i + 1] = a.normal.y; normal[3 * i + 2] = a.normal.z; }
          if (uv) { uv[2 * i] = a.u; uv[2 * i + 1] = a.v; }
          if (albedo) { albedo[3 * i] = a.albedo.x; albedo[3 * i + 1] = a.albedo.y; albedo[3 * i + 2] = a.albedo.z; }
          if (dir) { dir[3 * i] = a.dir.x; dir[3 * i + 1] = a.dir.y; dir[3 * i + 2] = a.dir.z; }
        }
    });
  for (std::thread& x : th) x.join();
  return 0;
}

// dr_accum_denoise on the host: the stage bodies of device_denoise.hpp over the pixel grid of settings13 (host_denoise_low, then the finish), from guides given
// as arrays in dr_render_aov's layout (normal / albedo gw x gh x 3, depth / material gw x gh) -- hk_aov's or the GPU's own.  acc: the column-major
// W x H x 3 accumulator; params: a dr_denoise_params (NULL: the defaults); out_f32 / out_rgb8 (either may be NULL): row-major W x H x 3.
// hist (may be NULL): the accumulator's history plane, W x H at x * H + y -- pixel p's divisor is hist[p] + divide_by.
// m2 (may be NULL): the second-moment plane, W x H at x * H + y -- option "denoise_variance" = 1: the variance pre-pass takes the temporal variance
// of pixels with four samples or more from it.  Returns 0, or -1 with hk_last_error.
int hk_denoise_m2(const int32_t* acc, int W, int H, int divide_by, const float* settings13, const float* normal, const float* albedo, const float* depth,
                  const int32_t* material, const int32_t* params, float* out_f32, uint8_t* out_rgb8, int nthreads, const int32_t* hist,
                  const unsigned long long* m2) {
  if (!acc || !settings13 || !normal || !albedo || !depth || !material) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(settings13, W, H, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  const DnParams D = params ? dn_params(params_from_words<dr_denoise_params>(params)) : DN_DEFAULTS;
  if (divide_by < 1) { hk_err = "denoise: divide_by must be >= 1"; return -1; }
  if (const char* why = check_denoise_params(D)) { hk_err = std::string("denoise: ") + why; return -1; }
  if (nthreads < 1) nthreads = 1;
  DnLaunch L;
  memset(&L, 0, sizeof(L));
  L.gw = P.gx * 8; L.gh = P.gy * 8; L.W = W; L.H = H; L.divide_by = divide_by;
  L.D = D;
  L.acc = acc; L.hist = hist; L.m2 = m2;
  L.normal = normal; L.depth = depth; L.albedo = albedo; L.mat = material;
  HostLow planes;
  if (D.iterations > 0) host_denoise_low(L, true, nthreads, planes);
  L.out_f32 = out_f32; L.out_rgb8 = out_rgb8;
  host_grid(nthreads, W, H, [&](int x, int y) { dn_finish_pixel(L, x, y); });
  return 0;
}

int hk_denoise(const int32_t* acc, int W, int H, int divide_by, const float* settings13, const float* normal, const float* albedo, const float* depth,
               const int32_t* material, const int32_t* params, float* out_f32, uint8_t* out_rgb8, int nthreads, const int32_t* hist) {
  return hk_denoise_m2(acc, W, H, divide_by, settings13, normal, albedo, depth, material, params, out_f32, out_rgb8, nthreads, hist, nullptr);
}

// dr_accum_upscale on the host: device_upscale.hpp over the output grid of settings13, from the low guides (the grid of settings13) and the full
// guides (settings13 with element 11 = 1) given as arrays in dr_render_aov's layout -- normal, albedo, depth, material each.  params: a
// dr_upscale_params (NULL: the defaults); prefilter: a dr_denoise_params or NULL -- the denoiser's host passes then run on the low grid first.
// out_f32 / out_rgb8 (either may be NULL): row-major W x H x 3; out_notap (may be NULL): W x H bytes, 1 where a guided pixel found no usable tap.
// hist / m2 as hk_denoise_m2.  Returns 0, or -1 with hk_last_error.
int hk_upscale(const int32_t* acc, int W, int H, int divide_by, const float* settings13, const float* normal, const float* albedo, const float* depth,
               const int32_t* material, const float* fnormal, const float* falbedo, const float* fdepth, const int32_t* fmaterial, const int32_t* params,
               const int32_t* prefilter, float* out_f32, uint8_t* out_rgb8, uint8_t* out_notap, int nthreads, const int32_t* hist,
               const unsigned long long* m2) {
  if (!acc || !settings13) { hk_err = "bad argument"; return -1; }
  RenderParams P, PF;
  memset(&P, 0, sizeof(P));
  memset(&PF, 0, sizeof(PF));
  if (const char* why = fill_view_params(settings13, W, H, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  float full13[13];
  memcpy(full13, settings13, sizeof(full13));
  full13[11] = 1.0f;
  if (const char* why = fill_view_params(full13, W, H, 0.0f, 0, 1, 0, PF)) { hk_err = why; return -1; }
  const UpParams UP = params ? up_params(params_from_words<dr_upscale_params>(params)) : UP_DEFAULTS;
  const DnParams PRE = prefilter ? dn_params(params_from_words<dr_denoise_params>(prefilter)) : DnParams{};
  const DnParams* const pre = prefilter ? &PRE : nullptr;
  if (divide_by < 1) { hk_err = "upscale: divide_by must be >= 1"; return -1; }
  hk_err = check_upscale_params(UP, pre);
  if (!hk_err.empty()) return -1;
  if (nthreads < 1) nthreads = 1;
  UpLaunch U;
  memset(&U, 0, sizeof(U));
  U.gw = P.gx * 8; U.gh = P.gy * 8; U.FW = PF.gx * 8; U.FH = PF.gy * 8; U.W = W; U.H = H;
  U.div = U.gw > 0 && U.gh > 0 ? (int)settings13[11] : 1; U.divide_by = divide_by;
  U.U = UP;
  U.acc = acc; U.hist = hist;
  HostLow low;
  std::vector<float> fguide, fgz;
  if (UP.mode == UP_GUIDED && U.gw > 0 && U.gh > 0) {
    if (!normal || !albedo || !depth || !material || !fnormal || !falbedo || !fdepth || !fmaterial) { hk_err = "bad argument"; return -1; }
    DnLaunch L;                                                             // the low side: the denoiser's planes
    memset(&L, 0, sizeof(L));
    L.gw = U.gw; L.gh = U.gh; L.W = W; L.H = H; L.divide_by = divide_by;
    L.D = up_low_params(UP, pre);
    L.acc = acc; L.hist = hist; L.m2 = m2;
    L.normal = normal; L.depth = depth; L.albedo = albedo; L.mat = material;
    host_denoise_low(L, pre != nullptr, nthreads, low);
    U.e = L.src; U.guide = L.guide; U.mat = L.mat;
    DnLaunch G;                                                             // the full side: the guide prepare over the full grid
    memset(&G, 0, sizeof(G));
    G.gw = U.FW; G.gh = U.FH;
    fguide.resize((size_t)4 * U.FW * U.FH); fgz.resize((size_t)U.FW * U.FH);
    G.normal = fnormal; G.depth = fdepth; G.mat = fmaterial; G.guide = fguide.data(); G.gz = fgz.data();
    host_grid(nthreads, G.gw, G.gh, [&](int x, int y) { dn_guide_pixel(G, x, y); });
    U.Fguide = G.guide; U.Falbedo = falbedo; U.Fmat = fmaterial; U.Fgz = G.gz;
  }
  U.out_f32 = out_f32; U.out_rgb8 = out_rgb8;
  host_grid(nthreads, W, H, [&](int X, int Y) {
    bool notap = false;
    up_pixel(U, X, Y, &notap);
    if (out_notap) out_notap[(size_t)Y * W + X] = notap ? 1 : 0;
  });
  return 0;
}

// The float camera block of a view as fill_view_params forms it (what dr_accum_reproject's definition starts from): out12 = from, llc, hor, ver;
// den2 = den_w, den_h; grid2 = gw, gh.  Returns 0, or -1 with hk_last_error.
int hk_camera_block(const float* settings13, int W, int H, float* out12, double* den2, int* grid2) {
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(settings13, W, H, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  memcpy(out12, P.from, 12); memcpy(out12 + 3, P.llc, 12); memcpy(out12 + 6, P.hor, 12); memcpy(out12 + 9, P.ver, 12);
  den2[0] = P.den_w; den2[1] = P.den_h;
  grid2[0] = P.gx * 8; grid2[1] = P.gy * 8;
  return 0;
}

// dr_accum_reproject on the host: device_reproject.hpp over the pixel grid, from guides given as arrays in dr_render_aov's layout (t / material
// gw x gh, normal gw x gh x 3) for both views -- hk_aov's or the GPU's own.  acc_from / acc_to: column-major W x H x 3; hist_from (may be NULL) /
// hist_to: W x H at x * H + y; params: a dr_reproject_params (NULL: the defaults); counts[5]: pixels, valid, masked, offscreen, rejected.
// m2_from / m2_to (both or neither NULL): the second-moment planes, W x H at x * H + y, carried with the sums (device_moments.hpp mo_carry).
// Returns 0, or -1 with hk_last_error.
int hk_reproject_m2(const int32_t* acc_from, const int32_t* hist_from, int W, int H, int frames, const float* from_settings13, const float* to_settings13,
                    const float* t_from, const float* normal_from, const int32_t* mat_from, const float* t_to, const float* normal_to, const int32_t* mat_to,
                    const int32_t* params, int32_t* acc_to, int32_t* hist_to, long long* counts, int nthreads, const unsigned long long* m2_from,
                    unsigned long long* m2_to) {
  if ((m2_from == nullptr) != (m2_to == nullptr)) { hk_err = "bad argument"; return -1; }
  if (!acc_from || !from_settings13 || !to_settings13 || !t_from || !normal_from || !mat_from || !t_to || !normal_to || !mat_to || !acc_to || !hist_to || !counts) { hk_err = "bad argument"; return -1; }
  RenderParams Pf, Pt;
  memset(&Pf, 0, sizeof(Pf)); memset(&Pt, 0, sizeof(Pt));
  if (const char* why = fill_view_params(from_settings13, W, H, 0.0f, 0, 1, 0, Pf)) { hk_err = why; return -1; }
  if (const char* why = fill_view_params(to_settings13, W, H, 0.0f, 0, 1, 0, Pt)) { hk_err = why; return -1; }
  if (Pf.gx != Pt.gx || Pf.gy != Pt.gy || Pf.den_w != Pt.den_w || Pf.den_h != Pt.den_h) { hk_err = "reproject: the two views have different divisors"; return -1; }
  if (frames < 1) { hk_err = "reproject: frames must be >= 1"; return -1; }
  RpLaunch L;
  memset(&L, 0, sizeof(L));
  L.R = params ? rp_params(params_from_words<dr_reproject_params>(params)) : RP_DEFAULTS;
  if (const char* why = check_reproject_params(L.R)) { hk_err = why; return -1; }
  fill_reproject_camera(Pt, L.to);
  fill_reproject_camera(Pf, L.from);
  if (!fill_reproject_proj(L.from, L.J)) { hk_err = "reproject: the `from` view is degenerate"; return -1; }
  L.gw = Pt.gx * 8; L.gh = Pt.gy * 8; L.W = W; L.H = H; L.frames = frames;
  L.t_to = t_to; L.normal_to = normal_to; L.mat_to = mat_to;
  L.t_from = t_from; L.normal_from = normal_from; L.mat_from = mat_from;
  L.acc_from = acc_from; L.hist_from = hist_from; L.acc_to = acc_to; L.hist_to = hist_to;
  L.m2_from = m2_from; L.m2_to = m2_to;
  memset(acc_to, 0, (size_t)W * H * 3 * sizeof(int32_t));                   // (pixels outside the grid: the body writes every pixel of the grid)
  memset(hist_to, 0, (size_t)W * H * sizeof(int32_t));
  if (m2_to) memset(m2_to, 0, (size_t)W * H * sizeof(unsigned long long));
  if (nthreads < 1) nthreads = 1;
  std::vector<long long> part((size_t)L.gh * 4, 0);                         // the classes of every row
  host_rows(nthreads, L.gh, [&](int y) {
    long long row[4] = {0, 0, 0, 0};
    for (int x = 0; x < L.gw; x++) row[rp_pixel(L, x, y)]++;
    memcpy(&part[(size_t)y * 4], row, sizeof(row));
  });
  counts[0] = (long long)L.gw * L.gh;
  for (int c = 0; c < 4; c++) { counts[1 + c] = 0; for (int y = 0; y < L.gh; y++) counts[1 + c] += part[(size_t)y * 4 + (size_t)c]; }
  return 0;
}

int hk_reproject(const int32_t* acc_from, const int32_t* hist_from, int W, int H, int frames, const float* from_settings13, const float* to_settings13,
                 const float* t_from, const float* normal_from, const int32_t* mat_from, const float* t_to, const float* normal_to, const int32_t* mat_to,
                 const int32_t* params, int32_t* acc_to, int32_t* hist_to, long long* counts, int nthreads) {
  return hk_reproject_m2(acc_from, hist_from, W, H, frames, from_settings13, to_settings13, t_from, normal_from, mat_from, t_to, normal_to, mat_to, params,
                         acc_to, hist_to, counts, nthreads, nullptr, nullptr);
}

// The fused add of the second-moment plane on the host (device_moments.hpp, as kernels_moments.hip runs it): acc += frame and m2 += the frame's capped
// luma squared, for npix pixels, in place.
int hk_moments_add(int32_t* acc, const int32_t* frame, unsigned long long* m2, long long npix) {
  if (!acc || !frame || !m2 || npix < 0) { hk_err = "bad argument"; return -1; }
  for (long long p = 0; p < npix; p++) mo_add_pixel(acc, frame, m2, (size_t)p);
  return 0;
}

// dr_accum_error on the host: device_moments.hpp over the pixel grid of settings13.  acc: column-major W x H x 3; hist (may be NULL) / m2: W x H at
// x * H + y; out_sigma (may be NULL): row-major W x H, 0 outside the grid; result (may be NULL): 19 words -- estimated, above, sum_var_q16, bins[16]
// (pixels = grid2[0] * grid2[1], returned in grid2).  Returns 0, or -1 with hk_last_error.
int hk_error(const int32_t* acc, const int32_t* hist, const unsigned long long* m2, int W, int H, int divide_by, float tolerance, const float* settings13,
             float* out_sigma, unsigned long long* result, int* grid2, int nthreads) {
  if (!acc || !m2 || !settings13 || (!out_sigma && !result)) { hk_err = "bad argument"; return -1; }
  RenderParams P;
  memset(&P, 0, sizeof(P));
  if (const char* why = fill_view_params(settings13, W, H, 0.0f, 0, 1, 0, P)) { hk_err = why; return -1; }
  if (divide_by < 0) { hk_err = "error: divide_by must be >= 0"; return -1; }
  if (!(tolerance >= 0.0f)) { hk_err = "error: tolerance must be >= 0"; return -1; }
  MoLaunch L;
  memset(&L, 0, sizeof(L));
  L.gw = P.gx * 8; L.gh = P.gy * 8; L.W = W; L.H = H; L.divide_by = divide_by; L.tolerance = tolerance;
  L.acc = acc; L.hist = hist; L.m2 = m2; L.out_sigma = out_sigma;
  if (grid2) { grid2[0] = L.gw; grid2[1] = L.gh; }
  if (out_sigma) memset(out_sigma, 0, (size_t)W * H * sizeof(float));
  if (nthreads < 1) nthreads = 1;
  std::vector<unsigned long long> part((size_t)L.gh * MO_WORDS, 0);         // the counts of every row
  host_rows(nthreads, L.gh, [&](int y) {
    unsigned long long cnt[MO_WORDS] = {0};
    for (int x = 0; x < L.gw; x++) {
      double var;
      float sigma;
      if (!mo_error_pixel(L, x, y, var, sigma)) continue;
      cnt[MO_ESTIMATED]++;
      if (sigma > L.tolerance) cnt[MO_ABOVE]++;
      cnt[MO_SUM_VAR] += mo_var_q16(var);
      cnt[MO_BIN0 + mo_bin(sigma)]++;
    }
    memcpy(&part[(size_t)y * MO_WORDS], cnt, sizeof(cnt));
  });
  if (result)
    for (int w = 0; w < MO_WORDS; w++) { result[w] = 0; for (int y = 0; y < L.gh; y++) result[w] += part[(size_t)y * MO_WORDS + (size_t)w]; }
  return 0;
}

}  // extern "C"
