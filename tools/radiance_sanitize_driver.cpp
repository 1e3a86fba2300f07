// The host build of dr_trace_radiance (tools/host_kernel.cpp hk_radiance) under AddressSanitizer + UBSan, as a stand-alone program: a few hundred random
// and degenerate rays with seeds and skips through every walk and both trees of every scene file given, against the sky and against every texture as
// the background.  Build and run from the repo root:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -mfma -pthread -DDR_HOST_BUILD=1 -I tools/host_kernel \
//     -o /tmp/radiance_asan tools/radiance_sanitize_driver.cpp tools/host_kernel.cpp dogeray_amd/csrc/{rts_reader,bvh_builder,linearise,wide_builder,capi_host}.cpp
//   /tmp/radiance_asan tests/golden/textures tests/golden/scenes/*.rts
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "host_kernel/hk_api.h"

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s TEXTURE_DIR scene.rts...\n", argv[0]); return 2; }
  const long long n = 600;
  uint64_t s = 88172645463325252ull;
  auto word = [&s]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  auto rnd = [&word]() { return (float)((double)(word() >> 11) * 0x1p-53); };
  const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, 1e-30f, 1e30f, std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::nanf("")};
  int bad = 0;
  for (int a = 2; a < argc; a++) {
    void* h = hk_scene_load(argv[a], argv[1]);
    if (!h) { printf("%s: not loaded (%s)\n", argv[a], hk_last_error()); continue; }
    std::vector<float> o(3 * n), d(3 * n), rad(3 * n);
    std::vector<uint64_t> seed(n);
    std::vector<int32_t> skip(n), bounces(n);
    for (long long i = 0; i < 3 * n; i++) {
      o[i] = (rnd() - 0.5f) * 20.0f; d[i] = rnd() - 0.5f;
      if (rnd() < 0.02f) o[i] = special[(int)(rnd() * 9) % 9];
      if (rnd() < 0.05f) d[i] = special[(int)(rnd() * 9) % 9];
    }
    for (long long i = 0; i < n; i++) { seed[i] = word(); skip[i] = (int32_t)(word() % 9); }
    // backtex -1, then textures 0, 1, .. until the scene refuses one
    for (int backtex = -1; backtex < 64; backtex++) {
      if (hk_radiance(h, 2, 2, 0, o.data(), d.data(), nullptr, nullptr, 1, 1, 1.0f, backtex, 0, rad.data(), nullptr) != 0) break;
      for (int tree = 1; tree <= 2; tree++)
        for (int traversal = 0; traversal <= 2; traversal++)
          for (int given = 0; given < 2; given++) {
            if (hk_radiance(h, traversal, tree, n, o.data(), d.data(), given ? seed.data() : nullptr, given ? skip.data() : nullptr, 3, 6, 0.75f, backtex, 99,
                            rad.data(), bounces.data()) != 0) { printf("%s: %s\n", argv[a], hk_last_error()); bad++; continue; }
            for (long long i = 0; i < n; i++) if (bounces[i] < 3 || bounces[i] > 18) { printf("%s: ray %lld: %d bounces\n", argv[a], i, bounces[i]); bad++; break; }
          }
    }
    hk_scene_free(h);
    printf("%s: ok\n", argv[a]);
  }
  return bad ? 1 : 0;
}
