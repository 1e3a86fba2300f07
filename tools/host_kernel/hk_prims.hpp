// Primitives and generator checks: the device functions of device_rng.hpp, device_intersect.hpp, device_surface.hpp, device_wide.hpp and device_shade.hpp on
// arrays of caller inputs, one pair per index, for the tests that pin them (no scene handle).  Part of host_kernel.cpp.
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
  for (long long i = 0; i < n; i++) out[i] = wide_ray_margin(ld3(o + 3 * i), ld3(d + 3 * i), e, l, v);
}
// the same with the certificate's factor (wide_ray_margin's last argument: 1e-4 / a_star for a certified camera ray, 1 otherwise)
void hk_ray_margin_k(long long n, const float* o, const float* d, float e, float l, float v, float k, float* out) {
  for (long long i = 0; i < n; i++) out[i] = wide_ray_margin(ld3(o + 3 * i), ld3(d + 3 * i), e, l, v, k);
}
// params_host.hpp cert_factor_k: the factor a certified camera ray carries for a_star
float hk_cert_factor_k(double a_star) { return cert_factor_k(a_star); }
// slab() (device_intersect.hpp: the reference's box test, what hk_camera_entry_check lists leaves with) on n ray / box pairs: 1 entered, 0 not
void hk_slab(long long n, const float* o, const float* d, const float* mn, const float* mx, int32_t* hit) {
  for (long long i = 0; i < n; i++) {
    const V3 dd = ld3(d + 3 * i);
    float dist = 0;
    hit[i] = slab(ld3(o + 3 * i), mk(1.0f / dd.x, 1.0f / dd.y, 1.0f / dd.z), mn + 3 * i, mx + 3 * i, dist) ? 1 : 0;
  }
}
// device_wide.hpp wide_pop and wide_pop_lean on n stack states (tests/test_lean_pop_host.py): state i is the register word top[i], the stack pointer sp[i]
// (0 .. WIDE_STACK, sb = 0) and WIDE_STACK stack words below it, stack[WIDE_STACK * i + k]; out[6 * i ..] = next record, remaining word, stack pointer of
// wide_pop, then the same three of wide_pop_lean
void hk_lean_pop(long long n, const uint32_t* top, const int32_t* sp, const uint32_t* stack, int32_t* out) {
  int lane_stack[WIDE_STACK * 64];
  for (long long i = 0; i < n; i++) {
    for (int form = 0; form < 2; form++) {
      for (int k = 0; k < WIDE_STACK; k++) lane_stack[k * 64] = (int)stack[WIDE_STACK * i + k];
      Trav tr; trav_begin(tr);
      WideStack ws; ws.top = top[i]; ws.sp = sp[i]; ws.sb = 0;
      if (form == 0) wide_pop(tr, ws, lane_stack);
      else wide_pop_lean(tr, ws, lane_stack);
      out[6 * i + 3 * form] = tr.node; out[6 * i + 3 * form + 1] = (int32_t)ws.top; out[6 * i + 3 * form + 2] = ws.sp;
    }
  }
}
// device_walk.hpp step_masks on n waves (tests/test_step_masks_host.py): wave i is the 64 lane words node[64 * i ..] (a record's link, or LANE_DONE /
// LANE_REFILL / LANE_RETIRED), from which the two ballots are formed as render_persistent_kernel's step_by_masks forms them -- walking and odd, walking and
// even --, with its flags draining[i], leaf_min[i], exclusive[i]; out[2 * i] = the lanes that step, out[2 * i + 1] = those of them that step as leaves
void hk_step_masks(long long n, const int32_t* node, const int32_t* draining, const int32_t* leaf_min, const int32_t* exclusive, uint64_t* out) {
  for (long long i = 0; i < n; i++) {
    unsigned long long on = 0ull, odd = 0ull;
    for (int l = 0; l < 64; l++) {
      if (node[64 * i + l] >= 0) on |= 1ull << l;
      if (node[64 * i + l] & 1) odd |= 1ull << l;
    }
    const StepMasks m = step_masks(on & odd, on & ~odd, draining[i] != 0, leaf_min[i], exclusive[i] != 0);
    out[2 * i] = m.step; out[2 * i + 1] = m.leaf;
  }
}
// hit_tri (device_intersect.hpp tri_hit) on n ray / triangle pairs: t or -1
void hk_tri_hit(long long n, const float* o, const float* d, const float* v0, const float* e1, const float* e2, float* t) {
  for (long long i = 0; i < n; i++)
    t[i] = tri_hit(ld3(o + 3 * i), ld3(d + 3 * i), ld3(v0 + 3 * i),
                   ld3(e1 + 3 * i), ld3(e2 + 3 * i));
}

// tri_hit's form that hands out the barycentrics (device_intersect.hpp): t or -1, and uv[2 i], uv[2 i + 1] as the test left them (0 where it never formed them)
void hk_tri_hit_uv(long long n, const float* o, const float* d, const float* v0, const float* e1, const float* e2, float* t, float* uv) {
  for (long long i = 0; i < n; i++) {
    float u = 0.0f, v = 0.0f;
    t[i] = tri_hit(ld3(o + 3 * i), ld3(d + 3 * i), ld3(v0 + 3 * i),
                   ld3(e1 + 3 * i), ld3(e2 + 3 * i), u, v);
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
}  // extern "C"
