// The host build of dr_trace_all_hits (tools/host_kernel.cpp hk_allhits, hk_allhits_brute) under AddressSanitizer + UBSan, as a stand-alone program: random,
// axis-parallel, huge and non-finite rays with adversarial tmax values through both walks and both trees of every scene file given, every list length
// from 0 to DR_ALLHITS_MAX and every kind mask, with every channel written, each against the brute-force definition.  Build and run from the repo root:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -mfma -pthread -DDR_HOST_BUILD=1 -I tools/host_kernel \
//     -o /tmp/allhits_asan tools/allhits_sanitize_driver.cpp tools/host_kernel.cpp dogeray_amd/csrc/{rts_reader,bvh_builder,linearise,wide_builder,capi_host}.cpp
//   /tmp/allhits_asan tests/golden/textures tests/golden/scenes/*.rts
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "host_kernel/hk_api.h"

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s TEXTURE_DIR scene.rts...\n", argv[0]); return 2; }
  const long long n = 1500;
  uint64_t s = 88172645463325252ull;
  auto rnd = [&s]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (float)((double)(s >> 11) * 0x1p-53); };
  const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, 1e-30f, 1e30f, 0x1p31f, std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::nanf("")};
  const int KM = hk_allhits_max();
  int bad = 0;
  for (int a = 2; a < argc; a++) {
    void* h = hk_scene_load(argv[a], argv[1]);
    if (!h) { printf("%s: not loaded (%s)\n", argv[a], hk_last_error()); continue; }
    std::vector<float> o(3 * n), d(3 * n), tmax(n);
    for (long long i = 0; i < 3 * n; i++) {
      o[i] = (rnd() - 0.5f) * 12.0f; d[i] = (rnd() - 0.5f) * 4.0f;
      if (rnd() < 0.03f) o[i] = special[(int)(rnd() * 10) % 10];
      if (rnd() < 0.08f) d[i] = special[(int)(rnd() * 10) % 10];
    }
    for (long long i = 0; i < n; i++) tmax[i] = rnd() < 0.2f ? special[(int)(rnd() * 10) % 10] : rnd() * 6.0f;
    for (int capped = 0; capped < 2; capped++)
      for (int K = 0; K <= KM; K++)
        for (int mask = 1; mask <= 3; mask++) {
          const float* cap = capped ? tmax.data() : nullptr;
          const size_t e = (size_t)n * (size_t)K;
          std::vector<int32_t> rc(n), ro(e + 1);
          std::vector<float> rt(e + 1);
          if (hk_allhits_brute(h, n, o.data(), d.data(), cap, K, mask, rc.data(), rt.data(), ro.data(), 2) != 0) { printf("%s: %s\n", argv[a], hk_last_error()); bad++; continue; }
          for (int tree = 1; tree <= 2; tree++)
            for (int walk = 0; walk <= 2; walk += 2) {
              // exactly-sized channels: a write past the end of a row is a heap overflow
              std::vector<int32_t> c(n), ob(e), mat(e), vis(n);
              std::vector<float> t(e), dist(e), nrm(3 * e), uv(2 * e), alb(3 * e);
              const bool k0 = K == 0;
              if (hk_allhits(h, walk, tree, n, o.data(), d.data(), cap, K, mask, 0, c.data(), k0 ? nullptr : t.data(), k0 ? nullptr : ob.data(), k0 ? nullptr : mat.data(),
                             k0 ? nullptr : dist.data(), k0 ? nullptr : nrm.data(), k0 ? nullptr : uv.data(), k0 ? nullptr : alb.data(), vis.data(), 2) != 0) {
                printf("%s: %s\n", argv[a], hk_last_error()); bad++; continue;
              }
              if (memcmp(c.data(), rc.data(), n * 4) || (e && (memcmp(t.data(), rt.data(), e * 4) || memcmp(ob.data(), ro.data(), e * 4)))) {
                printf("%s: walk %d tree %d K %d mask %d capped %d differs from the brute-force definition\n", argv[a], walk, tree, K, mask, capped); bad++;
              }
            }
        }
    hk_scene_free(h);
    printf("%s: ok\n", argv[a]);
  }
  return bad ? 1 : 0;
}
