#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <random>
#include "ldprune_hip_debug.h"
int main() {
  std::mt19937 rng(7);
  for (int iter = 0; iter < 60; ++iter) {
    const uint32_t m = 50 + rng() % 3000;
    const bool is_bp = rng() & 1;
    ldp_params P; memset(&P, 0, sizeof(P));
    P.founder_ct = 50 + rng() % 1000;
    P.window_is_bp = is_bp;
    P.prune_window_size = is_bp ? (500 + rng() % 50000) : (2 + rng() % 300);
    P.prune_window_incr = is_bp ? 1 : (1 + rng() % P.prune_window_size);
    P.prune_last_param = 0.5; P.plink1_order = rng() & 1; P.device = -1;
    ldp_engine* e = nullptr;
    if (ldp_create(&P, &e)) { printf("create failed\n"); return 1; }
    std::vector<uint32_t> chr(m), bp(m);
    uint32_t c = 0, pos = 1;
    for (uint32_t v = 0; v < m; ++v) { if (rng() % 400 == 0) { ++c; pos = 1; } pos += 1 + rng() % 300 + ((rng() % 100 == 0) ? 100000 : 0); chr[v] = c; bp[v] = pos; }
    int rc;
    const int mode = iter % 3;
    if (mode == 0) rc = ldp_set_variants(e, m, chr.data(), is_bp ? bp.data() : nullptr);
    else if (mode == 1) rc = ldp_set_variants_vcor(e, m, chr.data(), bp.data(), 1000 + rng() % 100000, 1 + rng() % 500);
    else rc = ldp_set_variants_matrix(e, m);
    if (rc) { printf("plan rc %d: %s\n", rc, ldp_last_error(e)); return 1; }
    // the passes over resident rows on an engine that has loaded nothing: random ranges (out of range and empty ones too) end in a return
    // code before the first device call, whatever the plan owns
    {
      const uint32_t fc = P.founder_ct;
      std::vector<uint32_t> c32a(fc), c32b(fc);
      std::vector<uint64_t> c64(fc), weight(m + 8);
      std::vector<uint8_t> flags(m + 8);
      std::vector<double> ln_p(m + 8);
      std::vector<ldp_king_counts_t> dense(static_cast<size_t>(8) * 8);
      std::vector<ldp_king_hit> hits(16);
      for (int t = 0; t < 24; ++t) {
        const uint32_t first = rng() % (m + 4);
        const uint32_t n = (t % 4 == 0) ? 0 : ((t % 4 == 1) ? rng() % 8 : rng() % (m + 4));
        const uint32_t row_first = rng() % fc, col_first = rng() % fc;
        uint64_t found = 0;
        int rcs[5];
        rcs[0] = ldp_sample_missing_counts(e, first, n, c32a.data());
        rcs[1] = ldp_sample_het_counts(e, first, n, nullptr, (t & 1) ? weight.data() : nullptr, c32a.data(), c32b.data(), (t & 1) ? c64.data() : nullptr);
        rcs[2] = ldp_king_counts_block(e, first, n, nullptr, row_first, 8, col_first, 8, dense.data(), 8);
        // (the hit form of an empty range with pairs goes on to the device: kept to ranges that refuse, or to blocks without a pair)
        rcs[3] = ldp_king_block_hits(e, first, n, nullptr, row_first, n ? 8 : 1, n ? col_first : row_first, n ? 8 : 1, 0.1, hits.data(), hits.size(), &found);
        rcs[4] = ldp_hwe_ln_pvals(e, first, n, t & 1, ln_p.data(), flags.data());
        for (int k = 0; k < 5; ++k) {
          if ((rcs[k] != LDP_OK) && (rcs[k] != LDP_ERR_STATE) && (rcs[k] != LDP_ERR_INVALID) && (rcs[k] != LDP_ERR_UNSUPPORTED)) {
            printf("resident pass %d on (%u, %u): rc %d: %s\n", k, first, n, rcs[k], ldp_last_error(e));
            return 1;
          }
        }
      }
    }
    std::vector<uint32_t> lo(m); uint64_t cand = 0;
    ldp_get_band(e, lo.data(), &cand);
    uint32_t sct = 0; ldp_get_subcontigs(e, &sct, nullptr, 0);
    if (mode == 0 && sct > 1 && (iter & 1)) { std::vector<uint32_t> owner(sct); ldp_set_shard(e, rng() % 3, 3, owner.data()); }
    if (mode == 0) {
      // replay over random true pairs inside the band
      std::vector<ldp_variant_rec> recs(m);
      memset(recs.data(), 0, recs.size() * sizeof(ldp_variant_rec));
      for (uint32_t v = 0; v < m; ++v) { recs[v].nm_ct = P.founder_ct; recs[v].ssq = 10; recs[v].sum = 1; }
      if (ldp_debug_set_variant_recs(e, recs.data()) == 0) {
        std::vector<double> mf(m); for (auto& x : mf) x = 0.5 + (rng() % 1000) / 2001.0;
        ldp_set_maj_freqs(e, 0, m, mf.data());
        std::vector<uint32_t> f, s2;
        for (uint32_t j = 1; j < m; ++j) if (lo[j] < j && rng() % 3 == 0) { f.push_back(lo[j] + rng() % (j - lo[j])); s2.push_back(j); }
        std::vector<uint64_t> removed((m + 63) / 64 + 1);
        const int drc = ldp_debug_replay_pairs(e, f.size(), f.data(), s2.data(), removed.data());
        // ... and through the CSR view of the same rows (option "replay_csr": block runs ascending / descending), whole and in three
        // instalments: the entries walked backwards, pred_word()'s search and the resume over them give the dense replay's words
        for (int view = 1; (view <= 2) && !drc; ++view) {
          for (int steps = 0; steps <= 3; steps += 3) {
            std::vector<uint64_t> again(removed.size());
            ldp_debug_set_option(e, "replay_csr", view);
            ldp_debug_set_option(e, "replay_steps", steps);
            const int rrc = ldp_debug_replay_pairs(e, f.size(), f.data(), s2.data(), again.data());
            if (rrc || (again != removed)) { printf("iter %d: replay_csr %d, replay_steps %d: rc %d, removed words differ from the dense replay's\n", iter, view, steps, rrc); return 1; }
          }
        }
        ldp_debug_set_option(e, "replay_csr", 0);
        ldp_debug_set_option(e, "replay_steps", 0);
      }
    }
    ldp_destroy(e);
  }
  printf("engine host logic: done\n");
  return 0;
}
