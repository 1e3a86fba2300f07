// The host build of dr_query_nearest (tools/host_kernel.cpp hk_nearest, hk_nearest_brute) under AddressSanitizer + UBSan, as a stand-alone program: random,
// huge and non-finite points with adversarial rmax values through both walks and both trees of every scene file given, each against the brute-force
// minimum.  Build and run from the repo root:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -mfma -pthread -DDR_HOST_BUILD=1 -I tools/host_kernel \
//     -o /tmp/nearest_asan tools/nearest_sanitize_driver.cpp tools/host_kernel.cpp dogeray_amd/csrc/{rts_reader,bvh_builder,linearise,wide_builder,capi_host}.cpp
//   /tmp/nearest_asan tests/golden/textures tests/golden/scenes/*.rts
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "host_kernel/hk_api.h"

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s TEXTURE_DIR scene.rts...\n", argv[0]); return 2; }
  const long long n = 2000;
  uint64_t s = 88172645463325252ull;
  auto rnd = [&s]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((double)(s >> 11) * 0x1p-53); };
  const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, 1e-30f, 1e30f, 0x1p31f, std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::nanf("")};
  int bad = 0;
  for (int a = 2; a < argc; a++) {
    void* h = hk_scene_load(argv[a], argv[1]);
    if (!h) { printf("%s: not loaded (%s)\n", argv[a], hk_last_error()); continue; }
    std::vector<float> p(3 * n), rmax(n);
    for (long long i = 0; i < 3 * n; i++) {
      p[i] = (rnd() - 0.5f) * 20.0f;
      if (rnd() < 0.03f) p[i] = special[(int)(rnd() * 10) % 10];
    }
    for (long long i = 0; i < n; i++) rmax[i] = rnd() < 0.15f ? special[(int)(rnd() * 10) % 10] : rnd() * 5.0f;
    struct Out { std::vector<float> dist, d2, pt, uv; std::vector<int32_t> obj, mat, vis; };
    auto make = [n]() { Out o; o.dist.resize(n); o.d2.resize(n); o.pt.resize(3 * n); o.uv.resize(2 * n); o.obj.resize(n); o.mat.resize(n); o.vis.resize(n); return o; };
    for (int capped = 0; capped < 2; capped++) {
      const float* cap = capped ? rmax.data() : nullptr;
      Out ref = make();
      if (hk_nearest_brute(h, n, p.data(), cap, ref.dist.data(), ref.d2.data(), ref.obj.data(), ref.mat.data(), ref.pt.data(), ref.uv.data(), 2) != 0) {
        printf("%s: %s\n", argv[a], hk_last_error()); bad++; continue;
      }
      for (int tree = 1; tree <= 2; tree++)
        for (int walk = 0; walk <= 2; walk += 2) {
          Out o = make();
          if (hk_nearest(h, walk, tree, n, p.data(), cap, o.dist.data(), o.d2.data(), o.obj.data(), o.mat.data(), o.pt.data(), o.uv.data(), o.vis.data(), 2) != 0) {
            printf("%s: %s\n", argv[a], hk_last_error()); bad++; continue;
          }
          if (memcmp(o.dist.data(), ref.dist.data(), n * 4) || memcmp(o.d2.data(), ref.d2.data(), n * 4) || memcmp(o.obj.data(), ref.obj.data(), n * 4) ||
              memcmp(o.mat.data(), ref.mat.data(), n * 4) || memcmp(o.pt.data(), ref.pt.data(), n * 12) || memcmp(o.uv.data(), ref.uv.data(), n * 8)) {
            printf("%s: walk %d tree %d capped %d differs from the brute-force minimum\n", argv[a], walk, tree, capped); bad++;
          }
        }
    }
    hk_scene_free(h);
    printf("%s: ok\n", argv[a]);
  }
  return bad ? 1 : 0;
}
