// Device functions of the temporal reprojection (dr_accum_reproject): the temporal half of SVGF (Schied et al. 2017) as a nearest-neighbour
// backward reprojection -- every pixel of the `to` view finds the pixel of the `from` view that saw the same surface point, validates it against
// the first-hit guides of both views (material, shading normal, plane distance) and carries its accumulated sums and sample count.
// Everything a pixel does is written once, here: rp_pixel takes the launch struct (RpLaunch, device_launch.h) and the pixel, classifies it,
// carries sums, history and M2 and writes the `to` pixel.  The gfx950 kernel (kernels_reproject.hip) maps a lane to a pixel, calls it and counts
// the classes per wave; the host build (tools/host_kernel.cpp hk_reproject) loops over the pixels, calls it and counts; tests/reproject_checks.py
// restates it in numpy float64 / int64, independently.  All of it is double on float inputs, only + - * /, sqrt,
// floor and comparisons, in the order written here (-ffp-contract=off): include/dogeray_amd.h has the definition this file implements,
// operation by operation.
#pragma once
#include "device_prims.hpp"      // the device or the host build's runtime (the one switch between them)
#include <stdint.h>

#include "device_launch.h"
#include "device_moments.hpp"

namespace dr {

struct D3 {
  double x, y, z;
};
__device__ __forceinline__ double rp_dot(const D3& a, const D3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ D3 rp_d3(const double* p) { D3 r; r.x = p[0]; r.y = p[1]; r.z = p[2]; return r; }
__device__ __forceinline__ D3 rp_f3(const float* p) { D3 r; r.x = (double)p[0]; r.y = (double)p[1]; r.z = (double)p[2]; return r; }

// The pinhole direction of pixel (x, y) as aov_first_hit (device_aov.hpp) forms it, in float: nu = (float)((x + 0.5) / den_w), nv likewise,
// d = ((llc + nu * hor) + nv * ver) - from per component; widened to double
__device__ __forceinline__ D3 rp_dir(const RpCamera& C, int x, int y) {
  const float nu = (float)(((double)x + 0.5) / C.den_w), nv = (float)(((double)y + 0.5) / C.den_h);
  D3 d;
  d.x = (double)(((C.llc[0] + nu * C.hor[0]) + nv * C.ver[0]) - C.from[0]);
  d.y = (double)(((C.llc[1] + nu * C.hor[1]) + nv * C.ver[1]) - C.from[1]);
  d.z = (double)(((C.llc[2] + nu * C.hor[2]) + nv * C.ver[2]) - C.from[2]);
  return d;
}

// the bit of material_mask that stands for material m: m itself for 0 .. 30, bit 31 for every other id
__device__ __forceinline__ bool rp_material_allowed(const RpParams& R, int m) {
  if (m == -1) return R.sky != 0;
  const int bit = (m < 0 || m > 31) ? 31 : m;
  return ((R.material_mask >> bit) & 1u) != 0;
}

// The class of pixel (x, y) of the `to` view, and for RP_VALID the pixel (qx, qy) of the `from` view it takes its history from.  The first-hit
// guides of both views are row-major planes of the gw x gh pixel grid as dr_render_aov writes them (pixel (x, y) at y * gw + x): t is hit()'s ray
// parameter (-1 on a miss), normal the shading normal (3 per pixel), mat the material (-1 on a miss).
//   masked     the material of p is not allowed (a miss: sky == 0)
//   offscreen  the world point lies behind the `from` camera's pinhole (a <= 0) or projects outside its pixel grid
//   rejected   the guides at q do not describe the same surface: another material, n_p . n_q < normal_cos, or X_q further than
//              plane_tolerance * |v| from the plane through X with normal n_p
__device__ __forceinline__ int rp_classify(const RpLaunch& L, int x, int y, int& qx, int& qy) {
  const RpParams& R = L.R;
  const RpCamera &to = L.to, &fr = L.from;
  const RpProj& J = L.J;
  const int gw = L.gw, gh = L.gh;
  const size_t p = (size_t)y * (size_t)gw + (size_t)x;
  const int mp = L.mat_to[p];
  if (!rp_material_allowed(R, mp)) return RP_MASKED;
  const bool miss = mp == -1;
  const D3 d = rp_dir(to, x, y);
  D3 X = d, v = d;                                     // a miss: the sky is at infinity, v = d
  if (!miss) {
    const double tp = (double)L.t_to[p];
    X.x = (double)to.from[0] + tp * d.x; X.y = (double)to.from[1] + tp * d.y; X.z = (double)to.from[2] + tp * d.z;
    v.x = X.x - (double)fr.from[0]; v.y = X.y - (double)fr.from[1]; v.z = X.z - (double)fr.from[2];
  }
  const D3 cN = rp_d3(J.cN), hor = rp_d3(J.hor), ver = rp_d3(J.ver);
  const double a = rp_dot(v, cN);
  if (!(a > 0.0)) return RP_OFFSCREEN;
  const double s = J.LcN / a;
  D3 r;
  r.x = s * v.x - J.L[0]; r.y = s * v.y - J.L[1]; r.z = s * v.z - J.L[2];
  const double nu = rp_dot(r, hor) / J.hh, nv = rp_dot(r, ver) / J.vv;
  const double fx = __builtin_floor(nu * fr.den_w), fy = __builtin_floor(nv * fr.den_h);
  if (!(fx >= 0.0 && fx < (double)gw && fy >= 0.0 && fy < (double)gh)) return RP_OFFSCREEN;
  qx = (int)fx; qy = (int)fy;
  const size_t q = (size_t)qy * (size_t)gw + (size_t)qx;
  if (L.mat_from[q] != mp) return RP_REJECTED;
  if (miss) return RP_VALID;
  const D3 np = rp_f3(L.normal_to + 3 * p), nq = rp_f3(L.normal_from + 3 * q);
  if (!(rp_dot(np, nq) >= (double)R.normal_cos)) return RP_REJECTED;
  const D3 dq = rp_dir(fr, qx, qy);
  const double tq = (double)L.t_from[q];
  D3 e;
  e.x = X.x - ((double)fr.from[0] + tq * dq.x); e.y = X.y - ((double)fr.from[1] + tq * dq.y); e.z = X.z - ((double)fr.from[2] + tq * dq.z);
  const double off = rp_dot(e, np), dist = off < 0.0 ? -off : off;
  if (!(dist <= (double)R.plane_tolerance * __builtin_sqrt(rp_dot(v, v)))) return RP_REJECTED;
  return RP_VALID;
}

// What a valid pixel carries: cnt = hist_q + frames samples; up to max_history of them as they are, beyond that the sums scaled to max_history
// samples (64-bit product, integer division towards zero)
__device__ __forceinline__ void rp_carry(const RpParams& R, int frames, const int32_t* acc_q, int hist_q, int32_t* acc_p, int32_t& hist_p) {
  const long long cnt = (long long)hist_q + (long long)frames;
  if (cnt <= (long long)R.max_history) {
    acc_p[0] = acc_q[0]; acc_p[1] = acc_q[1]; acc_p[2] = acc_q[2];
    hist_p = (int32_t)cnt;
  } else {
    acc_p[0] = (int32_t)(((long long)acc_q[0] * (long long)R.max_history) / cnt);
    acc_p[1] = (int32_t)(((long long)acc_q[1] * (long long)R.max_history) / cnt);
    acc_p[2] = (int32_t)(((long long)acc_q[2] * (long long)R.max_history) / cnt);
    hist_p = (int32_t)R.max_history;
  }
}

// Pixel (x, y) of the grid: its class; a valid pixel carries the sums, the sample count and (option "moments": the plane goes with the sums) M2 of
// the `from` pixel it projects to, every other pixel starts again at 0.  The accumulators are column-major W x H x 3 ((x * H + y) * 3), the
// history and second-moment planes W x H (x * H + y).
__device__ __forceinline__ int rp_pixel(const RpLaunch& L, int x, int y) {
  int qx = 0, qy = 0;
  const int cls = rp_classify(L, x, y, qx, qy);
  int32_t sums[3] = {0, 0, 0}, hist = 0;
  unsigned long long m2 = 0;
  if (cls == RP_VALID) {
    const size_t q = (size_t)qx * (size_t)L.H + (size_t)qy;
    const int32_t* aq = L.acc_from + q * 3;
    const int32_t from_sums[3] = {aq[0], aq[1], aq[2]};
    const int32_t hist_q = L.hist_from ? L.hist_from[q] : 0;
    rp_carry(L.R, L.frames, from_sums, hist_q, sums, hist);
    if (L.m2_to) m2 = mo_carry(L.m2_from[q], (long long)hist_q + (long long)L.frames, L.R.max_history);
  }
  const size_t p = (size_t)x * (size_t)L.H + (size_t)y;
  int32_t* ap = L.acc_to + p * 3;
  ap[0] = sums[0]; ap[1] = sums[1]; ap[2] = sums[2];
  L.hist_to[p] = hist;
  if (L.m2_to) L.m2_to[p] = m2;
  return cls;
}

}  // namespace dr
