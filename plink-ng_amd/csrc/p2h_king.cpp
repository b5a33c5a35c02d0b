// p2h_king.cpp -- plink2-hip: --make-king-table, the KING-robust kinship table (CalcKing, plink2_matrix_calc.cc:1662-2460) with
// --king-table-filter.  The reference runs it after every sample and variant filter over the autosomal variants the filters leave and every
// pair of kept samples.  Everything a line prints is a function of five integers of the pair -- variants where both samples are heterozygous,
// where one is heterozygous and the other homozygous (two counts), where both are homozygous, and where they are homozygous for different
// alleles --, so the two sources of those integers write the same bytes through the one writer here: the device's pass over the resident
// image (run_prune: ldp_king_counts_block / ldp_king_block_hits, p2h_prune.cpp) and the host's popcount pass over the rows (king_host_pass,
// p2h_inputs.cpp; king_pairs_host below).
//
// A line lists the LATER sample first, and the table's "1" in HET1_HOM2 / HET2_HOM1 is the line's SECOND sample, the earlier one (the writer
// loop :2284-2298 swaps them: "'2' here refers to the larger index"): HET1_HOM2 counts the variants where the earlier sample is heterozygous
// and the later one homozygous.
#include "p2h_cli.h"

namespace p2h {

void king_preamble(const Session& S, uint32_t sample_ct, uint32_t autosomal, uint32_t non_autosomal) {
  (void)S;
  if (sample_ct < 2) {  // :1682-1685 (kPglRetDegenerateData)
    die(13, "Error: --make-king-table requires at least 2 samples.\n");
  }
  if (non_autosomal) {  // :1704-1715
    logprintf("Excluding %u variant%s on non-autosomes from KING-robust calculation.\n", non_autosomal, (non_autosomal == 1) ? "" : "s");
    if (!autosomal) {
      die(13, "Error: No variants remaining for KING-robust calculation.\n");
    }
  }
}

KingWriter::KingWriter(const Session& S) : S_(S) {
  const Args& A = S.A;
  const uint32_t raw_sample_ct = static_cast<uint32_t>(S.is_founder.size());
  for (uint32_t sx = 0; sx < raw_sample_ct; ++sx) {
    if (S.sample_kept.empty() || S.sample_kept[sx]) {
      kept_.push_back(sx);
    }
  }
  const bool col_id = (A.king_cols & kKingColId) != 0;
  // FidColIsRequired / SidColIsRequired (plink2_common.h): 'fid' / 'sid' always, 'maybefid' / 'maybesid' when the fileset has the column
  col_fid_ = col_id && ((A.king_cols & kKingColFid) || ((A.king_cols & kKingColMaybefid) && S.fid_present));
  col_sid_ = col_id && ((A.king_cols & kKingColSid) || ((A.king_cols & kKingColMaybesid) && !S.sample_sids.empty()));
  if (col_id) {
    ids_.reserve(kept_.size());
    for (const uint32_t sx : kept_) {
      std::string id = S.sample_keys[sx].c_str() + (col_fid_ ? 0 : (S.sample_keys[sx].find('\t') + 1));  // ("FID<tab>IID"; FID "0" where the file has none)
      id += '\t';
      if (col_sid_) {
        id += S.sample_sids.empty() ? "0" : S.sample_sids[sx];
        id += '\t';
      }
      ids_.push_back(id);
    }
  }
  path_ = A.out + ".kin0" + (A.king_zs ? ".zst" : "");
  f_.open(path_, A.king_zs);
  // AppendKingTableHeader :1611-1652 (every title tab-terminated, the last tab becomes the line's end)
  buf_ = "#";
  if (col_id) {
    for (const char* k : {"1", "2"}) {
      if (col_fid_) {
        buf_ += std::string("FID") + k + "\t";
      }
      buf_ += std::string("IID") + k + "\t";
      if (col_sid_) {
        buf_ += std::string("SID") + k + "\t";
      }
    }
  }
  buf_ += (A.king_cols & kKingColNsnp) ? "NSNP\t" : "";
  buf_ += (A.king_cols & kKingColHethet) ? "HETHET\t" : "";
  buf_ += (A.king_cols & kKingColIbs0) ? "IBS0\t" : "";
  buf_ += (A.king_cols & kKingColIbs1) ? "HET1_HOM2\tHET2_HOM1\t" : "";
  buf_ += (A.king_cols & kKingColIbs) ? "IBS\t" : "";
  buf_ += (A.king_cols & kKingColKinship) ? "KINSHIP\t" : "";
  buf_.back() = '\n';
}

void KingWriter::pair(uint32_t row, uint32_t col, const ldp_king_counts_t& c) {
  const Args& A = S_.A;
  ++pairs_;
  // '2' is the larger index: het2hom1 = the later sample heterozygous (:2292-2298)
  const uint32_t ibs0_ct = c.ibs0, hethet_ct = c.hethet, het2hom1_ct = c.het_row_hom_col, het1hom2_ct = c.hom_row_het_col;
  const int64_t smaller_het_ct = static_cast<int64_t>(hethet_ct) + std::min(het1hom2_ct, het2hom1_ct);
  const double kinship = 0.5 - (static_cast<double>(4 * static_cast<int64_t>(ibs0_ct) + het1hom2_ct + het2hom1_ct) / static_cast<double>(4 * smaller_het_ct));
  if (A.king_filter_given && (kinship < A.king_filter)) {  // (-inf goes, NaN stays: :2303-2309)
    ++filtered_;
    return;
  }
  char num[64];
  auto put_u32 = [&](uint32_t v) { buf_.append(num, static_cast<size_t>(sprintf(num, "%u", v))); };
  auto put_g = [&](double v) { buf_.append(num, static_cast<size_t>(format_g6(v, num) - num)); };
  if (!ids_.empty()) {
    buf_ += ids_[row];
    buf_ += ids_[col];
  }
  const uint32_t nonmiss_ct = het1hom2_ct + het2hom1_ct + c.homhom + hethet_ct;
  const double nonmiss_recip = 1.0 / static_cast<double>(nonmiss_ct);
  if (A.king_cols & kKingColNsnp) {
    put_u32(nonmiss_ct);
    buf_ += '\t';
  }
  auto put = [&](uint32_t v) {
    if (A.king_counts) {
      put_u32(v);
    } else {
      put_g(nonmiss_recip * static_cast<double>(v));
    }
    buf_ += '\t';
  };
  if (A.king_cols & kKingColHethet) {
    put(hethet_ct);
  }
  if (A.king_cols & kKingColIbs0) {
    put(ibs0_ct);
  }
  if (A.king_cols & kKingColIbs1) {
    put(het1hom2_ct);
    put(het2hom1_ct);
  }
  if (A.king_cols & kKingColIbs) {
    const uint32_t hamming_dist = 2 * ibs0_ct + het1hom2_ct + het2hom1_ct;
    if (A.king_counts) {
      put_u32(hamming_dist);
    } else {
      put_g(nonmiss_recip * 0.5 * static_cast<double>(hamming_dist));
    }
    buf_ += '\t';
  }
  if (A.king_cols & kKingColKinship) {
    put_g(kinship);
    buf_ += '\t';
  }
  buf_.back() = '\n';
  if (buf_.size() > (1u << 20)) {
    f_.write(buf_.data(), buf_.size());
    buf_.clear();
  }
}

void KingWriter::finish(uint32_t variant_ct) {
  const Args& A = S_.A;
  f_.write(buf_.data(), buf_.size());
  buf_.clear();
  f_.close();
  logprintf("--make-king-table: %u variant%s processed.\n", variant_ct, (variant_ct == 1) ? "" : "s");
  if (!(A.king_cols & kKingColId)) {  // :2432-2442, WriteSampleIds (plink2_common.cc:4219-4270)
    const std::string id_path = A.out + ".kin0.id";
    FILE* f = fopen(id_path.c_str(), "wb");
    if (!f) {
      die(3, "Error: Failed to open %s for writing.\n", id_path.c_str());
    }
    fputs(S_.fid_present ? "#FID\tIID" : "#IID", f);
    fputs(S_.sample_sids.empty() ? "\n" : "\tSID\n", f);
    for (const uint32_t sx : kept_) {
      fputs(S_.sample_keys[sx].c_str() + (S_.fid_present ? 0 : 2), f);
      if (!S_.sample_sids.empty()) {
        fputc('\t', f);
        fputs(S_.sample_sids[sx].c_str(), f);
      }
      fputc('\n', f);
    }
    if (fclose(f)) {
      die(5, "Error: File write failure: %s.\n", id_path.c_str());
    }
    logprintf_ww("Results written to %s and %s .\n", path_.c_str(), id_path.c_str());
  } else {
    logprintf_ww("Results written to %s .\n", path_.c_str());
  }
  if (A.king_filter_given) {  // :2448-2452
    const uint64_t n = kept_.size();
    const uint64_t reported = n * (n - 1) / 2 - filtered_;
    logprintf("--king-table-filter: %llu relationship%s reported (%llu filtered out).\n", static_cast<unsigned long long>(reported), (reported == 1) ? "" : "s",
              static_cast<unsigned long long>(filtered_));
  }
}

void king_pairs_host(const std::vector<uint64_t>& het, const std::vector<uint64_t>& hom, const std::vector<uint64_t>& alt, size_t words, uint32_t sample_ct, uint32_t nthreads,
                     KingWriter* w) {
  // rows in batches of whole rows with about a quarter million pairs each; the batch's counts on the threads, its lines in order afterwards
  std::vector<ldp_king_counts_t> cts;
  for (uint32_t r0 = 1; r0 < sample_ct;) {
    uint32_t r1 = r0;
    uint64_t n_pairs = 0;
    while ((r1 < sample_ct) && ((r1 == r0) || (n_pairs + r1 <= (1u << 18)))) {
      n_pairs += r1;
      ++r1;
    }
    cts.resize(n_pairs);
    std::atomic<uint32_t> next(r0);
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < std::min<uint32_t>(nthreads, r1 - r0); ++t) {
      pool.emplace_back([&]() {
        for (uint32_t i = next.fetch_add(1); i < r1; i = next.fetch_add(1)) {
          // (rows r0 .. i - 1 hold r0 + ... + (i - 1) pairs)
          ldp_king_counts_t* out = cts.data() + (static_cast<uint64_t>(i) * (i - 1) / 2 - static_cast<uint64_t>(r0) * (r0 - 1) / 2);
          const uint64_t* ti = het.data() + static_cast<size_t>(i) * words;
          const uint64_t* hi = hom.data() + static_cast<size_t>(i) * words;
          const uint64_t* ai = alt.data() + static_cast<size_t>(i) * words;
          for (uint32_t j = 0; j < i; ++j) {
            const uint64_t* tj = het.data() + static_cast<size_t>(j) * words;
            const uint64_t* hj = hom.data() + static_cast<size_t>(j) * words;
            const uint64_t* aj = alt.data() + static_cast<size_t>(j) * words;
            uint32_t tt = 0, th = 0, ht = 0, hh = 0, i0 = 0;
            for (size_t k = 0; k < words; ++k) {
              const uint64_t both_hom = hi[k] & hj[k];
              tt += static_cast<uint32_t>(__builtin_popcountll(ti[k] & tj[k]));
              th += static_cast<uint32_t>(__builtin_popcountll(ti[k] & hj[k]));
              ht += static_cast<uint32_t>(__builtin_popcountll(hi[k] & tj[k]));
              hh += static_cast<uint32_t>(__builtin_popcountll(both_hom));
              i0 += static_cast<uint32_t>(__builtin_popcountll(both_hom & (ai[k] ^ aj[k])));
            }
            out[j] = ldp_king_counts_t{tt, th, ht, hh, i0};
          }
        }
      });
    }
    for (std::thread& th : pool) {
      th.join();
    }
    const ldp_king_counts_t* p = cts.data();
    for (uint32_t i = r0; i < r1; ++i) {
      for (uint32_t j = 0; j < i; ++j) {
        w->pair(i, j, *p++);
      }
    }
    r0 = r1;
  }
}

}  // namespace p2h
