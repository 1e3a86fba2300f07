// The camera rays' per-view grazing certificate and entry table: what one triangle, one leaf and one tile contribute.  All of it double and integer,
// none of it needs the vectors or the walks.
#pragma once
#include <stddef.h>
#include "device_layout.h"
#include "device_prims.hpp"

namespace dr {

// The tiles a box can be seen from: the second half of cert_leaf's rule, as a function of the box alone (rc = its centre - cv.from, h = its half extents
// with the slop in, rcn = |rc|, hn = |h|, fn = |cv.from|, cn = |centre|).  1 with rect, or 2 (every tile).  The camera rays' entry table asks it of
// every leaf (entry_leaf below).
// (ENTRY_MUTANT: a wrong rule on purpose, host build only -- tests/test_camera_entry_host.py shows that its cases catch each; device_prims.hpp)
__device__ __forceinline__ int cert_box_rect(const CertView& cv, const double* rc, const double* h, double rcn, double hn, double fn, double cn, int* rect) {
  const double zc = rc[0] * cv.w[0] + rc[1] * cv.w[1] + rc[2] * cv.w[2];
  const double zh = h[0] * __builtin_fabs(cv.w[0]) + h[1] * __builtin_fabs(cv.w[1]) + h[2] * __builtin_fabs(cv.w[2]);
  const double zmin = zc - zh, zmax = zc + zh;
  if (!(zmin > 2.0 * cv.r_o + 1e-9 * (fn + cn + hn) && zmin == zmin && zmax < 1e300)) return 2;
  double ulo = 1e300, uhi = -1e300, vlo = 1e300, vhi = -1e300;
  for (int k = 0; k < 8; k++) {
    double x[3];
    for (int a = 0; a < 3; a++) x[a] = rc[a] + (((k >> a) & 1) ? h[a] : -h[a]);
    const double z = x[0] * cv.w[0] + x[1] * cv.w[1] + x[2] * cv.w[2], s = cv.D / z;
    double pl[3];
    for (int a = 0; a < 3; a++) pl[a] = cv.from[a] + x[a] * s - cv.llc[a];
    const double nu = cv.du[0] * pl[0] + cv.du[1] * pl[1] + cv.du[2] * pl[2], nv = cv.dv[0] * pl[0] + cv.dv[1] * pl[1] + cv.dv[2] * pl[2];
    ulo = __builtin_fmin(ulo, nu); uhi = __builtin_fmax(uhi, nu); vlo = __builtin_fmin(vlo, nv); vhi = __builtin_fmax(vhi, nv);
  }
  const double rmax = rcn + hn;
  double lens = cv.r_o * (1.0 + (cv.D + cv.r_o) / (zmin - cv.r_o) + rmax * (cv.D + zmax) / (zmin * (zmin - cv.r_o)));
  if (ENTRY_MUTANT(2)) lens = 0.0;
  const double xlo = (ulo - cv.du_n * lens) * cv.den_w, xhi = (uhi + cv.du_n * lens) * cv.den_w;
  const double ylo = (vlo - cv.dv_n * lens) * cv.den_h, yhi = (vhi + cv.dv_n * lens) * cv.den_h;
  if (!(xlo == xlo && xhi == xhi && ylo == ylo && yhi == yhi)) return 2;
  auto pix = [](double f, int hi) { return f < -8.0 ? -8 : (f > (double)hi + 8.0 ? hi + 8 : (int)__builtin_floor(f)); };
  const int px0 = pix(xlo, cv.nx) - 2, px1 = pix(xhi, cv.nx) + 1, py0 = pix(ylo, cv.ny) - 2, py1 = pix(yhi, cv.ny) + 1;
  const int gc0 = (px0 < 0 ? 0 : px0) >> 3, gc1 = (px1 >= cv.nx ? cv.nx - 1 : px1) >> 3;
  rect[2] = (py0 < 0 ? 0 : py0) >> 3; rect[3] = (py1 >= cv.ny ? cv.ny - 1 : py1) >> 3;
  // global block columns [gc0, gc1] -> the launch's local columns (global = stripe_rem + local * stripe_mod)
  const int l0 = gc0 <= cv.stripe_rem ? 0 : (gc0 - cv.stripe_rem + cv.stripe_mod - 1) / cv.stripe_mod;
  const int l1 = gc1 < cv.stripe_rem ? -1 : (gc1 - cv.stripe_rem) / cv.stripe_mod;
  rect[0] = l0; rect[1] = l1 < cv.ncols - 1 ? l1 : cv.ncols - 1;
  if (px1 < 0 || py1 < 0 || px0 >= cv.nx || py0 >= cv.ny) rect[1] = rect[0] - 1;       // off the grid: no tile
  if (ENTRY_MUTANT(1)) { rect[0]++; rect[2]++; }
  return 1;
}

// The per-view grazing certificate of one triangle (CertView).  In double, for the triangle (v0, e1, e2) of a leaf:
//  * its padded box is taken as a superset of the reference's (own bounds + 0.01 (1 + 1e-4) + a rounding term per axis: K:353-354 pads v1, v2, v3 in double and
//    narrows, v0 + e1 is v1 up to one rounding of the edge), widened by what lets a float ray pass it while the real one misses (slab rounding; the float origin
//    and direction against the real ones of the same camera sample);
//  * every point X of that box and every origin O within r_o of `from`: |(X - O) . n| >= |(C - from) . n| - sum h_i |n_i| - r_o |n| and |X - O| <= |C - from| + |h| + r_o
//    (n = e1 x e2, C / h: the box's centre and half extents).  A float camera ray through X has d_f parallel to X - o_f, so
//    |a^| = |d_f . n| >= dmin (that numerator) / (that denominator): A_T, with a relative 1e-6 off for the double arithmetic;
//  * A_T >= a_star: 0 (certified).  Otherwise the tiles whose camera rays can pass the box: the box must lie in front of every lens point (else 2: every tile);
//    the pinhole images of its corners on the focus plane bound it from `from`, a lens offset moves an image by at most
//    r_o (1 + (D + r_o) / (zmin - r_o) + Rmax (D + zmax) / (zmin (zmin - r_o))); in pixels a sample's jitter adds one, the float nu another: 1 (rect = tile columns
//    [rect[0], rect[1]] of the LAUNCH and rows [rect[2], rect[3]]; an empty column range: none of the launch's tiles).
// Any NaN gives 1 with every tile, or 2.  A triangle that did not enter with its own bounds (|e1| |e2| > e_own) needs nothing: 0.
// Against a ladder (cv.level_a, ascending): *grade = the number of its steps A_T meets; all of them: 0 (the triangle constrains nobody), otherwise 1 / 2
// as above, the tiles of rect (every tile) having grade <= *grade.  The single step a_star (fill_cert_view) is the rule above.
__device__ __forceinline__ int cert_leaf(const CertView& cv, const float* v0f, const float* e1f, const float* e2f, int* rect, int* grade = nullptr) {
  double v0[3], e1[3], e2[3];
  for (int a = 0; a < 3; a++) { v0[a] = v0f[a]; e1[a] = e1f[a]; e2[a] = e2f[a]; }
  const double n1 = __builtin_sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), n2 = __builtin_sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
  if (grade) *grade = cv.n_levels;
  if (!(n1 * n2 <= cv.e_own)) return 0;
  double c[3], h[3], rc[3], n[3];
  double cn = 0, hn = 0;
  for (int a = 0; a < 3; a++) {
    const double p = v0[a] + e1[a], q = v0[a] + e2[a];
    const double lo = __builtin_fmin(v0[a], __builtin_fmin(p, q)), hi = __builtin_fmax(v0[a], __builtin_fmax(p, q));
    const double pad = 0.01 * 1.0001 + 0x1p-22 * (__builtin_fabs(v0[a]) + __builtin_fabs(e1[a]) + __builtin_fabs(e2[a]) + 1.0);
    c[a] = 0.5 * (lo + hi); h[a] = 0.5 * (hi - lo) + pad;
    cn += c[a] * c[a]; hn += h[a] * h[a];
  }
  cn = __builtin_sqrt(cn); hn = __builtin_sqrt(hn);
  const double fn = __builtin_sqrt(cv.from[0] * cv.from[0] + cv.from[1] * cv.from[1] + cv.from[2] * cv.from[2]);
  double rcn = 0;
  for (int a = 0; a < 3; a++) { rc[a] = c[a] - cv.from[a]; rcn += rc[a] * rc[a]; }
  rcn = __builtin_sqrt(rcn);
  const double slop = 0x1p-19 * (cn + hn + fn + 1.0) + cv.eps_d * (rcn + hn + cv.r_o) / cv.dmin;
  hn = 0;
  for (int a = 0; a < 3; a++) { h[a] += slop; hn += h[a] * h[a]; }
  hn = __builtin_sqrt(hn);
  n[0] = e1[1] * e2[2] - e1[2] * e2[1]; n[1] = e1[2] * e2[0] - e1[0] * e2[2]; n[2] = e1[0] * e2[1] - e1[1] * e2[0];
  const double nn = __builtin_sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  const double num = __builtin_fabs(rc[0] * n[0] + rc[1] * n[1] + rc[2] * n[2]) - (h[0] * __builtin_fabs(n[0]) + h[1] * __builtin_fabs(n[1]) + h[2] * __builtin_fabs(n[2])) - cv.r_o * nn;
  const double den = rcn + hn + cv.r_o;
  const double a_t = num > 0.0 ? cv.dmin * (num / den) * (1.0 - 1e-6) : 0.0;
  int g = 0;
  while (g < cv.n_levels && a_t >= cv.level_a[g]) g++;
  if (grade) *grade = g;
  if (g == cv.n_levels) return 0;
  return cert_box_rect(cv, rc, h, rcn, hn, fn, cn, rect);      // flagged: the tiles its box can be seen from
}

// ---- the camera rays' entry table (option camera_entry): one record per tile at which the tile's camera rays start their walk
// instead of the root -- the lowest record of the wide tree that has every leaf a camera ray of the tile can reach under it.  "Can reach": the leaf's
// box, the reference's padded one of its record (units A and B) widened by cert_leaf's slop, can be seen from the tile (cert_box_rect).  Leaves are
// numbered in depth-first order (linearise.hpp WideImage: rank), so the leaves under a record are one run of ranks and a tile only needs the lowest and
// the highest rank that reach it.  The table while it is built, mm: word 2 t = the lowest rank of tile t, word 2 t + 1 = ~ the highest (both start at
// all ones and only ever fall: one kind of atomic); word 2 ntiles falls to 0 when some leaf sends every tile to the root.
// An entry code is a walk's `node` word: record << 1 | is-leaf, 0 = the root, ENTRY_NONE (-1: nothing to walk) for a tile no leaf can be seen from.

// the tiles the box [mn, mx] of a leaf record can be seen from: 1 with rect, or 2 (every tile: not in front of the lens, or a NaN)
__device__ __forceinline__ int entry_box_rect(const CertView& cv, const float* mn, const float* mx, int* rect) {
  double c[3], h[3], rc[3];
  double cn = 0, hn = 0, rcn = 0;
  for (int a = 0; a < 3; a++) {
    const double lo = mn[a], hi = mx[a];
    c[a] = 0.5 * (lo + hi); h[a] = 0.5 * (hi - lo) + 0x1p-50 * (__builtin_fabs(lo) + __builtin_fabs(hi));      // (the sum and the difference round once each)
    rc[a] = c[a] - cv.from[a];
    cn += c[a] * c[a]; hn += h[a] * h[a]; rcn += rc[a] * rc[a];
  }
  cn = __builtin_sqrt(cn); hn = __builtin_sqrt(hn); rcn = __builtin_sqrt(rcn);
  const double fn = __builtin_sqrt(cv.from[0] * cv.from[0] + cv.from[1] * cv.from[1] + cv.from[2] * cv.from[2]);
  const double slop = 0x1p-19 * (cn + hn + fn + 1.0) + cv.eps_d * (rcn + hn + cv.r_o) / cv.dmin;      // cert_leaf's
  hn = 0;
  for (int a = 0; a < 3; a++) { h[a] += slop; hn += h[a] * h[a]; }
  hn = __builtin_sqrt(hn);
  return cert_box_rect(cv, rc, h, rcn, hn, fn, cn, rect);
}
// the leaf of rank `rank` with the box [mn, mx] folded into mm
__device__ __forceinline__ void entry_leaf(const CertView& cv, const float* mn, const float* mx, uint32_t rank, uint32_t* __restrict__ mm, int ntiles) {
  int rect[4] = {0, -1, 0, -1};
  if (entry_box_rect(cv, mn, mx, rect) == 2) { entry_min(&mm[2 * (size_t)ntiles], 0u); return; }
  const uint32_t top = ENTRY_MUTANT(3) && rank > 0u ? rank - 1u : rank;
  for (int col = rect[0]; col <= rect[1]; col++)
    for (int r = rect[2]; r <= rect[3]; r++) {
      const size_t t = (size_t)col * (size_t)cv.gy + (size_t)r;
      entry_min(&mm[2 * t], rank); entry_min(&mm[2 * t + 1], ~top);
    }
}
// the entry code of a tile whose leaves have the ranks [lo, ~hi_inv]: down from the root while one child holds them all.  range: two words per
// record, the ranks of the leaves under it.  (Siblings' ranges are disjoint: at most one child holds a non-empty run.)
__device__ __forceinline__ int entry_tile(const DevUnit* __restrict__ wide, const uint32_t* __restrict__ range, uint32_t lo, uint32_t hi_inv, bool every) {
  if (every) return 0;
  if (lo == 0xffffffffu) return ENTRY_NONE;
  const uint32_t hi = ~hi_inv;
  if (ENTRY_MUTANT(4) && lo == hi) return ENTRY_NONE;
  uint32_t cur = 0u;
  for (int level = 0; level < WIDE_MAX_DEPTH; level++) {
    const uint32_t w = reinterpret_cast<const uint32_t*>(wide + (size_t)cur * WIDE_UNITS)[3];
    const uint32_t base = w & 0xffffffu, valid = (w >> 24) & 15u, leafmask = w >> 28;
    int next = -1;
    for (int k = 0; k < 4; k++) {
      const size_t ch = (size_t)base + (size_t)k;
      if (((valid >> k) & 1u) && range[2 * ch] <= lo && hi <= range[2 * ch + 1]) next = k;
    }
    if (next < 0) break;
    if ((leafmask >> next) & 1u) return (int)(((base + (uint32_t)next) << 1) | 1u);
    cur = base + (uint32_t)next;
  }
  return (int)(cur << 1);
}

}  // namespace dr
