// The host build of the shading step's known-answer hooks (tools/host_kernel.cpp hk_kat_*: device_kat_shade.hpp over device_rng.hpp, device_surface.hpp
// and device_shade.hpp) under AddressSanitizer + UBSan, as a stand-alone program: random and non-finite rays, texture coordinates, directions and colours
// through every hook, on every object and texture of every scene file given.  Build and run from the repo root:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -mfma -pthread -DDR_HOST_BUILD=1 -I tools/host_kernel \
//     -o /tmp/shade_asan tools/shade_sanitize_driver.cpp tools/host_kernel.cpp dogeray_amd/csrc/{rts_reader,bvh_builder,linearise,wide_builder,capi_host}.cpp
//   /tmp/shade_asan tests/golden/textures tests/golden/scenes/*.rts
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "host_kernel/hk_api.h"

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s TEXTURE_DIR scene.rts...\n", argv[0]); return 2; }
  const long long n = 4000;
  uint64_t s = 88172645463325252ull;
  auto word = [&s]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  auto rnd = [&word]() { return (float)((double)(word() >> 11) * 0x1p-53); };
  const float inf = std::numeric_limits<float>::infinity();
  const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, 1e-30f, 1e30f, inf, -inf, std::nanf(""), 8421504.0f, 8421505.0f, -8421505.0f};
  auto value = [&](float scale) { return rnd() < 0.05f ? special[(int)(rnd() * 12) % 12] : (rnd() - 0.5f) * scale; };
  int bad = 0;
  // the hooks that read no scene
  std::vector<uint64_t> seed(n);
  std::vector<int32_t> warm(n), kind(n), xs(n), ys(n), smp(n), out3(3 * n), flag(n);
  std::vector<float> p1(3 * n), p2(3 * n), v3(3 * n), o6(6 * n), d6(6 * n);
  std::vector<uint32_t> n1(2 * n), n2(2 * n), n4(4 * n);
  for (long long i = 0; i < n; i++) {
    seed[i] = word(); warm[i] = (int32_t)(word() % 9); kind[i] = (int32_t)(i % 4 == 0 ? 0 : (i % 4 == 1 ? 2 : 3));
    xs[i] = (int32_t)word(); ys[i] = (int32_t)word(); smp[i] = (int32_t)(word() % 7);
  }
  for (float& f : v3) f = value(6.0f);
  if (hk_kat_sample(n, seed.data(), warm.data(), kind.data(), p1.data(), n1.data(), p2.data(), n2.data()) != 0) bad++;
  if (hk_kat_outside(3 * n, v3.data(), out3.data()) != 0) bad++;
  if (hk_kat_store(n, v3.data(), 1, out3.data()) != 0 || hk_kat_store(n, v3.data(), 3, out3.data()) != 0) bad++;
  const float st[13] = {7.3f, -6.9f, 4.9f, 0, 0, 0, 0.6f, 9.5f, 45, 5, 4, 1, -1};
  if (hk_kat_camera(st, 320, 192, 0xffffffffffffffffull, 0x02000001u, n, xs.data(), ys.data(), smp.data(), o6.data(), d6.data(), n4.data()) != 0) bad++;
  for (int a = 2; a < argc; a++) {
    void* h = hk_scene_load(argv[a], argv[1]);
    if (!h) { printf("%s: not loaded (%s)\n", argv[a], hk_last_error()); continue; }
    // objects and textures: as many as the scene answers for (the hooks refuse an index out of range)
    int32_t zero = 0;
    float f0[3] = {0, 0, 1}, f1[3] = {0, 0, -1}, one[3] = {1, 1, 1}, tt = 1.0f, res3[6];
    uint64_t sd = 1; int32_t al[2]; uint32_t nx[4], texel;
    int n_obj = 0, n_tex = 0;
    for (int32_t k = 0; k < 100000; k++, n_obj++) if (hk_kat_bounce(h, 1, &k, f0, f1, &tt, one, &sd, &zero, al, res3, res3, res3, nx) != 0) break;
    for (int32_t k = 0; k < 64; k++, n_tex++) if (hk_kat_tex(h, 1, &k, &tt, &tt, &texel) != 0) break;
    std::vector<int32_t> obj(n), tex(n), alive(2 * n);
    std::vector<float> o(3 * n), d(3 * n), t(n), at(3 * n), u(n), v(n), a6(6 * n), rgb(3 * n);
    std::vector<uint32_t> texels(n);
    for (long long i = 0; i < n; i++) {
      obj[i] = (int32_t)(word() % (uint64_t)n_obj); tex[i] = n_tex ? (int32_t)(word() % (uint64_t)n_tex) : 0;
      t[i] = value(10.0f); u[i] = value(8.0f); v[i] = value(8.0f);
      for (int k = 0; k < 3; k++) { o[3 * i + k] = value(20.0f); d[3 * i + k] = value(2.0f); at[3 * i + k] = rnd(); }
    }
    if (n_obj > 0 && hk_kat_bounce(h, n, obj.data(), o.data(), d.data(), t.data(), at.data(), seed.data(), warm.data(), alive.data(), o6.data(), d6.data(),
                                   a6.data(), n4.data()) != 0) { printf("%s: %s\n", argv[a], hk_last_error()); bad++; }
    if (n_tex > 0 && hk_kat_tex(h, n, tex.data(), u.data(), v.data(), texels.data()) != 0) { printf("%s: %s\n", argv[a], hk_last_error()); bad++; }
    for (int bt = -1; bt < n_tex; bt++)
      if (hk_kat_miss(h, n, d.data(), at.data(), bt, 0.75f, rgb.data()) != 0) { printf("%s: %s\n", argv[a], hk_last_error()); bad++; }
    hk_scene_free(h);
    printf("%s: %d objects, %d textures: ok\n", argv[a], n_obj, n_tex);
  }
  return bad ? 1 : 0;
}
