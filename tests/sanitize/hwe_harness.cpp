// AddressSanitizer + UndefinedBehaviorSanitizer over ldp_hwe_ln_p_host (csrc/ldp_hwe_host.cpp, csrc/ldp_hwe_core.h), stand-alone, no GPU:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off -Iinclude \
//       tests/sanitize/hwe_harness.cpp plink-ng_amd/csrc/ldp_hwe_host.cpp -o /tmp/hwe_harness && /tmp/hwe_harness
// Every triple with n <= 24, the corners of the 31-bit range (where the 64-bit products of a step are largest) and an oversized triple;
// prints a checksum so that the calls cannot be optimised away.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "ldprune_hip.h"

int main() {
  double sum = 0.0;
  unsigned flagged = 0;
  uint8_t f = 0;
  for (uint32_t n = 0; n <= 24; ++n) {
    for (uint32_t a = 0; a <= n; ++a) {
      for (uint32_t b = 0; a + b <= n; ++b) {
        for (int midp = 0; midp < 2; ++midp) {
          sum += ldp_hwe_ln_p_host(a, b, n - a - b, midp, &f);
          flagged += f;
        }
      }
    }
  }
  const uint32_t big = 0x7fffffffu;
  const uint32_t corners[][3] = {{big, 0, 0}, {0, big, 0}, {0, 0, big}, {big / 2, 0, big - big / 2}, {big / 2, 1, big / 2}, {big - 3, 2, 1}, {1, 2, big - 3},
                                 {big / 2 - 50000, 100001, big / 2 - 50000}, {1000000, big - 2000000, 1000000}};
  for (const auto& c : corners) {
    // (the all-het corner walks 2^30 steps: leave it to a smaller one of the same shape)
    const uint32_t het = (c[1] == big) ? 2000001u : c[1];
    sum += ldp_hwe_ln_p_host(c[0], het, c[2], 0, &f) + ldp_hwe_ln_p_host(c[0], het, c[2], 1, nullptr);
    flagged += f;
  }
  const double bad = ldp_hwe_ln_p_host(big, big, 0, 0, &f);
  if (!std::isnan(bad) || (f != 0x80)) {
    fprintf(stderr, "an oversized triple was not refused\n");
    return 1;
  }
  printf("checksum %.17g, %u flagged\n", sum, flagged);
  return 0;
}
