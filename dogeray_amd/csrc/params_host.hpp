// settings[13] -> the per-launch constants of RenderParams that do not depend on the device: the camera block of Kernel
// (kernel.cu K:1016-1052, identical for every pixel, so evaluated once on the host with the reference's float / double promotions),
// the sample scale, the block grid and the stripe; and the parameter sets of the accumulator stages (dr_denoise_params, dr_upscale_params,
// dr_reproject_params): their defaults, their ranges and their device form, each written here and nowhere else.  Host only; shared by the
// context_*.cpp files and the host build of the kernel arithmetic (tools/host_kernel.cpp).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/dogeray_amd.h"
#include "device_launch.h"

namespace dr {

struct V3h { float x, y, z; };
inline V3h hsub(V3h a, V3h b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3h hmul(V3h a, V3h b) { return {a.x * b.x, a.y * b.y, a.z * b.z}; }
inline V3h hdiv(V3h a, V3h b) { return {a.x / b.x, a.y / b.y, a.z / b.z}; }
inline V3h hsplat(float a) { return {a, a, a}; }
inline float hdot(V3h a, V3h b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3h hcross(V3h a, V3h b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline V3h hnorm(V3h v) { float inv = 1.0f / sqrtf(hdot(v, v)); return {v.x * inv, v.y * inv, v.z * inv}; }
inline void st3(float* d, V3h v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; }
inline int hf2i(float f) {       // float -> int as CUDA's cvt.rzi.s32.f32: saturating, NaN -> 0
  if (f != f) return 0;
  if (f >= 2147483648.0f) return 2147483647;
  if (f <= -2147483648.0f) return (-2147483647 - 1);
  return (int)f;
}

// Fills the camera, sampling and grid fields of P (everything else is left as it is).  Returns null, or what is wrong with the arguments.
inline const char* fill_view_params(const float* st, int W, int H, float background, uint64_t seed, int stripe_mod, int stripe_rem, RenderParams& P) {
  if (W <= 0 || H <= 0 || W > 65000 || H > 65000 || (size_t)W * (size_t)H > (size_t)1 << 28) return "bad frame size";      // (x and y share a word in the phase stash)
  const int div = hf2i(st[11]);
  if (div < 1) return "divisor must be >= 1";
  float aspect = float(W / st[11]) / float(H / st[11]);           // K:1016 (int / float)
  float fov = (float)((double)st[8] * M_PI / 180);                // K:1020
  float vh = (float)(2.0 * (double)tanf(fov / 2));                // K:1023
  float vw = aspect * vh;
  V3h from = {st[0], st[1], st[2]}, at = {st[3], st[4], st[5]};
  float focus = st[7];
  V3h vup = {0, 1, 0};
  V3h wu = hnorm(hsub(from, at));
  V3h uu = hnorm(hcross(vup, wu));
  V3h vu = hcross(wu, uu);
  V3h hor = hmul(hmul(hsplat(focus), hsplat(vw)), uu);            // K:1047
  V3h ver = hmul(hmul(hsplat(focus), hsplat(vh)), vu);
  V3h llc = hsub(hsub(hsub(from, hdiv(hor, hsplat(2))), hdiv(ver, hsplat(2))), hmul(hsplat(focus), wu));
  st3(P.from, from); st3(P.llc, llc); st3(P.hor, hor); st3(P.ver, ver); st3(P.uu, uu); st3(P.vu, vu);
  P.lens_radius = st[6] / 2;                                      // K:1052
  P.bgint = background;
  P.spp_f = st[10];
  P.scale = (float)(1.0 / (double)st[10]);                        // K:1081
  P.den_w = (double)float(W / st[11]);                            // K:1067
  P.den_h = (double)float(H / st[11]);
  P.seed = seed;
  P.W = W; P.H = H;
  P.gx = W / div / 8; P.gy = H / div / 8;                         // K:2636
  P.stripe_mod = stripe_mod; P.stripe_rem = stripe_rem;
  P.ncols = P.gx > stripe_rem ? (P.gx - stripe_rem + stripe_mod - 1) / stripe_mod : 0;
  P.seed_stride = 8u * (unsigned)P.gx;                            // blockDim.x * gridDim.x, K:1065
  P.max_depth = hf2i(st[9]);
  P.backtex = hf2i(st[12]);
  P.batch = 1;
  P.batch_seed_stride = 0;
  P.sample_magic = 0;                                             // (one frame: both sample orders are the identity)
  return nullptr;
}

// The camera rays' grazing certificate of a view (CertView, device_layout.h; device_cert.hpp cert_leaf): from the launch's float camera block, in double.
// a_star: the certified |a^| (>= 1e-4); e_own: the scene's WideMu e.  Returns false when the view gives nothing to certify with (no own-bounds tree,
// degenerate camera, non-finite values): its camera rays then keep the scene's margin.
inline bool fill_cert_view(const RenderParams& P, double a_star, float e_own, CertView& cv) {
  memset(&cv, 0, sizeof(cv));
  if (!(e_own > 0.0f) || !(a_star >= 1e-4)) return false;
  double hor[3], ver[3], uu[3], vu[3];
  for (int a = 0; a < 3; a++) { cv.from[a] = P.from[a]; cv.llc[a] = P.llc[a]; hor[a] = P.hor[a]; ver[a] = P.ver[a]; uu[a] = P.uu[a]; vu[a] = P.vu[a]; }
  auto dot = [](const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
  auto norm = [&](const double* a) { return std::sqrt(dot(a, a)); };
  double w[3] = {hor[1] * ver[2] - hor[2] * ver[1], hor[2] * ver[0] - hor[0] * ver[2], hor[0] * ver[1] - hor[1] * ver[0]};
  const double wn = norm(w);
  if (!(wn > 0) || !std::isfinite(wn)) return false;
  double lf[3] = {cv.llc[0] - cv.from[0], cv.llc[1] - cv.from[1], cv.llc[2] - cv.from[2]};
  for (int a = 0; a < 3; a++) w[a] /= wn;
  if (dot(lf, w) < 0) for (int a = 0; a < 3; a++) w[a] = -w[a];
  memcpy(cv.w, w, sizeof(w));
  cv.D = dot(lf, w);
  const double hh = dot(hor, hor), hv = dot(hor, ver), vv = dot(ver, ver), det = hh * vv - hv * hv;
  if (!(det > 0)) return false;
  for (int a = 0; a < 3; a++) { cv.du[a] = (vv * hor[a] - hv * ver[a]) / det; cv.dv[a] = (hh * ver[a] - hv * hor[a]) / det; }
  cv.du_n = norm(cv.du); cv.dv_n = norm(cv.dv);
  const double r = std::fabs((double)P.lens_radius), fn = norm(cv.from);
  // lens offset uu rd.x + vu rd.y with |rd.x|, |rd.y| <= r (a point of the unit disk, times r, rounded), and the float sum from + offset
  cv.r_o = 1.001 * r * (norm(uu) + norm(vu)) + 0x1p-22 * (fn + 2.0 * r) + 1e-30;
  // d_f = llc + nu hor + nv ver - from - offset (0 <= nu, nv <= 1): two products and four sums, each rounded once per component
  cv.eps_d = 0x1p-20 * (norm(cv.llc) + norm(hor) + norm(ver) + fn + cv.r_o);
  // |d| >= d . w = D + nu hor . w + nv ver . w - offset . w (hor, ver are orthogonal to w up to the double rounding)
  cv.dmin = cv.D - cv.r_o - 1e-9 * (norm(hor) + norm(ver)) - cv.eps_d;
  cv.den_w = P.den_w; cv.den_h = P.den_h;
  cv.a_star = a_star;
  cv.level_a[0] = a_star; cv.n_levels = 1; cv.base = 0;      // (the single step; cert_ladder sets the graded one)
  cv.e_own = (double)e_own * (1.0 + 1e-6);
  cv.nx = 8 * P.gx; cv.ny = 8 * P.gy; cv.gy = P.gy;
  cv.stripe_mod = P.stripe_mod; cv.stripe_rem = P.stripe_rem; cv.ncols = P.ncols;
  const double all[] = {cv.D, cv.r_o, cv.eps_d, cv.dmin, cv.du_n, cv.dv_n, fn};
  for (double v : all) if (!std::isfinite(v)) return false;
  // (a view whose focus plane is not clearly in front of the lens certifies nothing)
  return cv.dmin > 8.0 * cv.r_o && cv.dmin > 0;
}

// Temporal reprojection (dr_accum_reproject): a view's float camera block, and the projection into it in double -- L = llc - from,
// cN = hor x ver (negated when cN . L < 0), L . cN, hor . hor, ver . ver, every dot product (a.x b.x + a.y b.y) + a.z b.z.  Returns false
// for a degenerate view: L . cN zero or not finite.
inline void fill_reproject_camera(const RenderParams& P, RpCamera& C) {
  for (int a = 0; a < 3; a++) { C.from[a] = P.from[a]; C.llc[a] = P.llc[a]; C.hor[a] = P.hor[a]; C.ver[a] = P.ver[a]; }
  C.den_w = P.den_w; C.den_h = P.den_h;
}
inline bool fill_reproject_proj(const RpCamera& C, RpProj& J) {
  auto dot = [](const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
  for (int a = 0; a < 3; a++) { J.L[a] = (double)C.llc[a] - (double)C.from[a]; J.hor[a] = (double)C.hor[a]; J.ver[a] = (double)C.ver[a]; }
  J.cN[0] = J.hor[1] * J.ver[2] - J.hor[2] * J.ver[1];
  J.cN[1] = J.hor[2] * J.ver[0] - J.hor[0] * J.ver[2];
  J.cN[2] = J.hor[0] * J.ver[1] - J.hor[1] * J.ver[0];
  if (dot(J.cN, J.L) < 0) for (int a = 0; a < 3; a++) J.cN[a] = -J.cN[a];
  J.LcN = dot(J.L, J.cN);
  J.hh = dot(J.hor, J.hor); J.vv = dot(J.ver, J.ver);
  return std::isfinite(J.LcN) && J.LcN != 0.0;
}
// The defaults of the three parameter sets, in their device form (dr_*_defaults hand them out field by field)
constexpr DnParams DN_DEFAULTS = {5, 4.0f, 7, 1.0f, 1, 1};
constexpr UpParams UP_DEFAULTS = {UP_GUIDED, 5, 1.0f, 1, 1};
constexpr RpParams RP_DEFAULTS = {32, 0.9f, 0.01f, 0xFFFFFFC3u, 1};
// The device form of a parameter set: the same fields, every flag 0 or 1
inline DnParams dn_params(const dr_denoise_params& p) {
  return {p.iterations, p.sigma_luminance, p.normal_power_log2, p.sigma_depth, p.demodulate != 0, p.material_stop != 0};
}
inline UpParams up_params(const dr_upscale_params& p) { return {p.mode, p.normal_power_log2, p.sigma_depth, p.demodulate != 0, p.material_stop != 0}; }
inline RpParams rp_params(const dr_reproject_params& p) { return {p.max_history, p.normal_cos, p.plane_tolerance, p.material_mask, p.sky != 0}; }

// dr_denoise_params' ranges; null, or what is wrong (the caller says whose parameters they are)
inline const char* check_denoise_params(const DnParams& D) {
  if (D.iterations < 0 || D.iterations > DN_MAX_ITERATIONS) return "iterations must be 0 .. 10";
  if (!(D.sigma_luminance >= 0.0f) || !(D.sigma_depth >= 0.0f)) return "sigma_luminance and sigma_depth must be >= 0";
  if (D.normal_power_log2 < 0 || D.normal_power_log2 > DN_MAX_NORMAL_POWER_LOG2) return "normal_power_log2 must be 0 .. 16";
  return nullptr;
}
// dr_upscale_params' ranges, and a prefilter (null: none) judged against them; empty, or what is wrong
inline std::string check_upscale_params(const UpParams& U, const DnParams* prefilter) {
  if (U.mode != UP_BLOCK && U.mode != UP_GUIDED) return "upscale: mode must be DR_UPSCALE_BLOCK or DR_UPSCALE_GUIDED";
  if (U.normal_power_log2 < 0 || U.normal_power_log2 > DN_MAX_NORMAL_POWER_LOG2) return "upscale: normal_power_log2 must be 0 .. 16";
  if (!(U.sigma_depth >= 0.0f)) return "upscale: sigma_depth must be >= 0";
  if (!prefilter) return "";
  if (U.mode == UP_BLOCK) return "upscale: a prefilter needs the guided mode (dr_accum_denoise filters without upscaling)";
  if (const char* why = check_denoise_params(*prefilter)) return std::string("upscale: prefilter ") + why;
  if (prefilter->iterations < 1) return "upscale: prefilter iterations must be >= 1";
  if (prefilter->demodulate != U.demodulate) return "upscale: prefilter demodulate differs from the upscale parameters'";
  return "";
}
// The denoiser's parameters on the upsampler's low side: the prefilter's (its demodulate is the upscale parameters'), or without one what colour
// stage 0 reads of them
inline DnParams up_low_params(const UpParams& U, const DnParams* prefilter) {
  return prefilter ? *prefilter : DnParams{0, 0.0f, 0, 0.0f, U.demodulate, U.material_stop};
}
// dr_reproject_params' ranges; null, or what is wrong
inline const char* check_reproject_params(const RpParams& R) {
  if (R.max_history < 1 || R.max_history > RP_MAX_HISTORY) return "reproject: max_history must be 1 .. 65535";
  if (!(R.normal_cos >= -1.0f && R.normal_cos <= 1.0f)) return "reproject: normal_cos must be -1 .. 1";
  if (!(R.plane_tolerance >= 0.0f)) return "reproject: plane_tolerance must be >= 0";
  return nullptr;
}

// The judges of the accumulator stages' calls, one per stage, run by the library (context_accum.cpp) and by the host build (tools/host_kernel/
// hk_accum.hpp) alike.  A judge is given the caller's arguments and the view(s) as fill_view_params filled them; it checks what needs no device, in
// the order the library refuses, and fills the launch struct (zeroed first) with the grid, the sizes and the parameters -- the caller adds the
// pointers.  Returns the refusal, or "".

// settings13 at full resolution (element 11 = 1): the upsampler's second view
inline void full_view13(const float* settings13, float* full13) {
  memcpy(full13, settings13, 13 * sizeof(float));
  full13[11] = 1.0f;
}
// the denoiser's launch over the pixel grid of view P: dr_accum_denoise's, and the low side of dr_accum_upscale
inline DnLaunch low_launch(const RenderParams& P, int divide_by, const DnParams& D) {
  DnLaunch L;
  memset(&L, 0, sizeof(L));
  L.gw = P.gx * 8; L.gh = P.gy * 8; L.W = P.W; L.H = P.H; L.divide_by = divide_by; L.D = D;
  return L;
}
inline std::string judge_denoise(const RenderParams& P, int divide_by, const dr_denoise_params* params, DnLaunch& L) {
  if (divide_by < 1) return "denoise: divide_by must be >= 1";
  const DnParams D = params ? dn_params(*params) : DN_DEFAULTS;
  if (const char* why = check_denoise_params(D)) return std::string("denoise: ") + why;
  L = low_launch(P, divide_by, D);
  return "";
}
// P: the view of settings13, PF: of its full_view13.  L is the low side (run by a guided call on a grid that is not empty; its passes when there is a prefilter)
inline std::string judge_upscale(const RenderParams& P, const RenderParams& PF, const float* settings13, int divide_by, const dr_upscale_params* params,
                                 const dr_denoise_params* prefilter, UpLaunch& U, DnLaunch& L) {
  if (divide_by < 1) return "upscale: divide_by must be >= 1";
  const UpParams UP = params ? up_params(*params) : UP_DEFAULTS;
  const DnParams PRE = prefilter ? dn_params(*prefilter) : DnParams{};
  const DnParams* const pre = prefilter ? &PRE : nullptr;
  const std::string why = check_upscale_params(UP, pre);
  if (!why.empty()) return why;
  memset(&U, 0, sizeof(U));
  U.gw = P.gx * 8; U.gh = P.gy * 8; U.FW = PF.gx * 8; U.FH = PF.gy * 8; U.W = P.W; U.H = P.H;
  U.div = U.gw > 0 && U.gh > 0 ? (int)settings13[11] : 1; U.divide_by = divide_by;
  U.U = UP;
  L = low_launch(P, divide_by, up_low_params(UP, pre));
  return "";
}
// Pf, Pt: the `from` and the `to` view.  The judge's first check is a function of its own: the library makes it ahead of its context's checks
// (stripe, accumulator size), which stand before the judge's other refusals in dr_accum_reproject's order
inline const char* check_reproject_views(const RenderParams& Pf, const RenderParams& Pt) {
  if (Pf.gx != Pt.gx || Pf.gy != Pt.gy || Pf.den_w != Pt.den_w || Pf.den_h != Pt.den_h) return "reproject: the two views have different divisors";
  return nullptr;
}
inline std::string judge_reproject(const RenderParams& Pf, const RenderParams& Pt, int frames, const dr_reproject_params* params, RpLaunch& L) {
  if (const char* why = check_reproject_views(Pf, Pt)) return why;
  if (frames < 1) return "reproject: frames must be >= 1";
  memset(&L, 0, sizeof(L));
  L.R = params ? rp_params(*params) : RP_DEFAULTS;
  if (const char* why = check_reproject_params(L.R)) return why;
  fill_reproject_camera(Pt, L.to);
  fill_reproject_camera(Pf, L.from);
  if (!fill_reproject_proj(L.from, L.J)) return "reproject: the `from` view is degenerate (its focus plane has no normal facing the camera)";
  L.gw = Pt.gx * 8; L.gh = Pt.gy * 8; L.W = Pt.W; L.H = Pt.H; L.frames = frames;
  return "";
}
inline std::string judge_error(const RenderParams& P, int divide_by, float tolerance, MoLaunch& L) {
  if (divide_by < 0) return "error: divide_by must be >= 0";
  if (!(tolerance >= 0.0f)) return "error: tolerance must be >= 0";
  memset(&L, 0, sizeof(L));
  L.gw = P.gx * 8; L.gh = P.gy * 8; L.W = P.W; L.H = P.H; L.divide_by = divide_by; L.tolerance = tolerance;
  return "";
}

// dr_render_adaptive: the defaults, the ranges and the pass's launch over the tile grid of view P
constexpr AdParams AD_DEFAULTS = {1.0f, 4, 0, 1};
inline AdParams ad_params(const dr_adaptive_params& p) { return {p.tolerance, p.min_samples, p.max_samples, p.tile_pixels}; }
inline const char* check_adaptive_params(const AdParams& A) {
  if (!(A.tolerance >= 0.0f)) return "adaptive: tolerance must be >= 0";
  if (A.min_samples < 2) return "adaptive: min_samples must be >= 2";
  if (A.max_samples != 0 && A.max_samples <= A.min_samples) return "adaptive: max_samples must be 0 or > min_samples";
  if (A.tile_pixels < 1 || A.tile_pixels > 64) return "adaptive: tile_pixels must be 1 .. 64";
  return nullptr;
}
inline std::string judge_adaptive(const RenderParams& P, int nframes, int divide_by, const dr_adaptive_params* params, AdLaunch& L) {
  if (nframes < 1) return "adaptive: nframes must be >= 1";
  if (divide_by < 0) return "adaptive: divide_by must be >= 0";
  const AdParams A = params ? ad_params(*params) : AD_DEFAULTS;
  if (const char* why = check_adaptive_params(A)) return why;
  memset(&L, 0, sizeof(L));
  L.gx = P.gx; L.gy = P.gy; L.W = P.W; L.H = P.H; L.divide_by = divide_by; L.A = A; L.nframes = nframes;
  return "";
}

// The certificate's ladder for option cert_factor (CertView level_a, ascending; a_star stays level_a[base] = 1e-4 cert_factor): graded, cert_factor x
// {1/4, 1/2, 1, 2, 4}, each step at least the 1e-4 cut-off itself (the lemma needs a_star >= 1e-4); otherwise the single step cert_factor.
inline void cert_ladder(int cert_factor, bool graded, CertView& cv) {
  const double mult[5] = {0.25, 0.5, 1.0, 2.0, 4.0};
  cv.n_levels = graded ? 5 : 1; cv.base = graded ? 2 : 0;
  for (int g = 0; g < cv.n_levels; g++) {
    const double f = (double)cert_factor * (graded ? mult[g] : 1.0);
    cv.level_a[g] = 1e-4 * (f > 1.0 ? f : 1.0);
  }
}

// The factor a certified camera ray's |d|-proportional margin carries: 1e-4 / a_star, rounded up (step 2 divides by a_star instead of 1e-4)
inline float cert_factor_k(double a_star) {
  const double x = 1e-4 / a_star;
  float f = (float)x;
  if ((double)f < x) f = std::nextafter(f, INFINITY);
  return f;
}

}  // namespace dr
