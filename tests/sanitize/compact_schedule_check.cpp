// The batch schedule of the in-place row compaction (plink-ng_amd/csrc/ldp_compact_schedule.h, what ldp_restrict_variants() runs its copy
// kernel by) on a few thousand random keep masks and batch lengths, executed on a model image: a row is its original index.  Checked:
//   * no batch that is copied directly has overlapping source and destination ranges,
//   * every row that has to move is written exactly once, a row of the prefix that stays never,
//   * nothing is read after its slot was overwritten, and the bounce buffer never holds more than one batch,
//   * the image ends up as the kept rows in order.
// Stand-alone, CPU only:  c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined compact_schedule_check.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../plink-ng_amd/csrc/ldp_compact_schedule.h"

#define CHECK(cond)                                                                                         \
  do {                                                                                                      \
    if (!(cond)) {                                                                                          \
      fprintf(stderr, "compact_schedule_check: %s failed (line %d; case %u: %u rows, %u kept, batch %u)\n", #cond, __LINE__, it, n_old, n_kept, batch); \
      return 1;                                                                                             \
    }                                                                                                       \
  } while (0)

int main(int argc, char** argv) {
  const uint32_t cases = (argc > 1) ? static_cast<uint32_t>(atoi(argv[1])) : 4000;
  std::mt19937_64 rng(20240607);
  uint64_t direct_batches = 0, bounce_batches = 0;
  for (uint32_t it = 0; it < cases; ++it) {
    const uint32_t n_old = static_cast<uint32_t>(rng() % 700);
    uint32_t batch = static_cast<uint32_t>(1 + rng() % 40);
    if (it % 17 == 0) {
      batch = static_cast<uint32_t>(rng() % 3) * 1000;  // 0 (treated as 1), 1000, 2000: longer than the image
    }
    // keep masks of every kind: dense, sparse, a prefix that stays, one run dropped, everything, nothing
    std::vector<uint32_t> src;
    const uint32_t kind = static_cast<uint32_t>(rng() % 6);
    const double p = static_cast<double>(rng() % 1001) / 1000.0;
    const uint32_t cut = n_old ? static_cast<uint32_t>(rng() % n_old) : 0, run = static_cast<uint32_t>(rng() % 60);
    for (uint32_t v = 0; v < n_old; ++v) {
      bool keep;
      switch (kind) {
        case 0: keep = true; break;
        case 1: keep = false; break;
        case 2: keep = (v < cut) || (v >= cut + run); break;
        case 3: keep = (v < cut) || (static_cast<double>(rng() % 1000) / 1000.0 < p); break;
        case 4: keep = (v != 0); break;
        default: keep = static_cast<double>(rng() % 1000) / 1000.0 < p; break;
      }
      if (keep) {
        src.push_back(v);
      }
    }
    const uint32_t n_kept = static_cast<uint32_t>(src.size());
    std::vector<ldp::CompactBatch> sched;
    ldp::compact_schedule(src.data(), n_kept, batch, &sched);
    std::vector<uint32_t> image(n_old);
    std::vector<uint8_t> overwritten(n_old, 0);
    std::vector<uint32_t> writes(n_old, 0);
    for (uint32_t v = 0; v < n_old; ++v) {
      image[v] = v;
    }
    std::vector<uint32_t> bounce(batch ? batch : 1);
    uint32_t next = 0;
    while ((next < n_kept) && (src[next] == next)) {
      ++next;
    }
    for (const ldp::CompactBatch& b : sched) {
      CHECK(b.k0 == next && b.k1 > b.k0 && b.k1 <= n_kept);  // ascending, gapless, behind the prefix that stays
      CHECK(b.k1 - b.k0 <= bounce.size());
      next = b.k1;
      if (!b.bounce) {
        ++direct_batches;
        CHECK(b.k1 <= src[b.k0]);  // destination rows [k0, k1) end at or before the first source row
        for (uint32_t k = b.k0; k < b.k1; ++k) {
          CHECK(src[k] >= b.k1 && src[k] < n_old && !overwritten[src[k]]);
        }
        for (uint32_t k = b.k0; k < b.k1; ++k) {  // (any order: the ranges are disjoint)
          image[k] = image[src[k]];
          overwritten[k] = 1;
          ++writes[k];
        }
      } else {
        ++bounce_batches;
        for (uint32_t k = b.k0; k < b.k1; ++k) {
          CHECK(src[k] < n_old && !overwritten[src[k]]);
          bounce[k - b.k0] = image[src[k]];
        }
        for (uint32_t k = b.k0; k < b.k1; ++k) {
          image[k] = bounce[k - b.k0];
          overwritten[k] = 1;
          ++writes[k];
        }
      }
    }
    CHECK(next == n_kept || sched.empty());
    for (uint32_t k = 0; k < n_kept; ++k) {
      CHECK(image[k] == src[k]);
      CHECK(writes[k] == ((src[k] == k) ? 0u : 1u));
    }
    for (uint32_t v = n_kept; v < n_old; ++v) {
      CHECK(writes[v] == 0);
    }
  }
  printf("compact schedule: %u cases, %llu direct and %llu bounced batches, clean\n", cases, static_cast<unsigned long long>(direct_batches),
         static_cast<unsigned long long>(bounce_batches));
  return (direct_batches && bounce_batches) ? 0 : 1;
}
