// p2h_inputs.cpp -- plink2-hip: chromosome / sample filters and load_inputs(): everything the commands share (one translation unit of the front-end; plink2_hip_cli.cpp has the overview)
#include "p2h_cli.h"

#include <optional>

namespace p2h {

// --chr / --not-chr / --autosome: a chromosome's numeric code (1..22, X 23, Y 24, XY 25, MT 26, 0; -1 for other names)
int chrom_code(const std::string& name_in) {
  std::string name = name_in;
  if (name.size() > 3 && (name[0] | 32) == 'c' && (name[1] | 32) == 'h' && (name[2] | 32) == 'r') {
    name = name.substr(3);
  }
  bool numeric = !name.empty();
  for (char c : name) {
    numeric = numeric && (c >= '0' && c <= '9');
  }
  if (numeric) {
    const long v = strtol(name.c_str(), nullptr, 10);
    return (v <= 26) ? static_cast<int>(v) : -1;
  }
  if (ieq(name.c_str(), "X")) return 23;
  if (ieq(name.c_str(), "Y")) return 24;
  if (ieq(name.c_str(), "XY")) return 25;
  if (ieq(name.c_str(), "MT") || ieq(name.c_str(), "M")) return 26;
  return -1;
}

// is chromosome `name` named by one of the --chr style terms ("7", "chr7", "3-9", "X", "contig_12")?
bool chrom_listed(const std::vector<std::string>& terms, const std::string& name) {
  const int code = chrom_code(name);
  std::string bare = name;
  if (bare.size() > 3 && (bare[0] | 32) == 'c' && (bare[1] | 32) == 'h' && (bare[2] | 32) == 'r') {
    bare = bare.substr(3);
  }
  for (const std::string& t : terms) {
    const size_t dash = t.find('-');
    if ((dash != std::string::npos) && (dash > 0) && (dash + 1 < t.size())) {
      const int lo = chrom_code(t.substr(0, dash)), hi = chrom_code(t.substr(dash + 1));
      if ((lo >= 0) && (hi >= lo)) {
        if ((code >= lo) && (code <= hi)) {
          return true;
        }
        continue;
      }
    }
    const int tc = chrom_code(t);
    if (tc >= 0) {
      if (tc == code) {
        return true;
      }
      continue;
    }
    std::string tb = t;
    if (tb.size() > 3 && (tb[0] | 32) == 'c' && (tb[1] | 32) == 'h' && (tb[2] | 32) == 'r') {
      tb = tb.substr(3);
    }
    if (tb == bare) {
      return true;
    }
  }
  return false;
}

std::vector<std::string> tokens_of_file(const std::string& path) {
  const std::string text = slurp(path);
  std::vector<std::string> out;
  for (size_t p0 = 0; p0 < text.size();) {
    while ((p0 < text.size()) && (static_cast<unsigned char>(text[p0]) <= ' ')) {
      ++p0;
    }
    size_t p1 = p0;
    while ((p1 < text.size()) && (static_cast<unsigned char>(text[p1]) > ' ')) {
      ++p1;
    }
    if (p1 > p0) {
      out.emplace_back(text, p0, p1 - p0);
    }
    p0 = p1;
  }
  return out;
}

// --keep / --remove files (LoadXidHeader + LoadSampleIds, plink2_common.cc:1313,1707): "FID<tab>IID" keys.  A header line
// "#FID IID ..." or "#IID ..." names the columns; without one, a line of two or more tokens is FID IID and a line of one is
// an IID with FID "0".
void load_sample_id_list(const std::string& path, const char* flag, std::vector<std::string>* keys) {
  std::ifstream in(path);
  if (!in) {
    die(3, "Error: Failed to open %s.\n", path.c_str());
  }
  std::string line;
  int mode = 0;  // 0: no header (FID IID or IID), 1: #FID IID, 2: #IID
  bool first = true;
  size_t line_idx = 0;
  while (std::getline(in, line)) {
    ++line_idx;
    std::vector<std::string> t = split_ws(line);
    if (t.empty()) {
      continue;
    }
    if (t[0][0] == '#') {
      if (first && ((t[0] == "#FID") || (t[0] == "#IID"))) {
        first = false;
        if (t[0] == "#FID") {
          if ((t.size() < 2) || (t[1] != "IID")) {
            die(6, "Error: No IID column on line %zu of --%s file.\n", line_idx, flag);
          }
          mode = 1;
        } else {
          mode = 2;
        }
        if ((t.size() > static_cast<size_t>(3 - mode)) && (t[3 - mode] == "SID")) {
          die(63, "Error: SID columns in --%s files are not supported by plink2-hip.\n", flag);
        }
      }
      continue;  // (other '#' lines before the data are comments)
    }
    first = false;
    if (mode == 2) {
      keys->push_back("0\t" + t[0]);
    } else if ((mode == 1) || (t.size() >= 2)) {
      if (t.size() < 2) {
        die(6, "Error: Line %zu of --%s file has fewer tokens than expected.\n", line_idx, flag);
      }
      keys->push_back(t[0] + "\t" + t[1]);
    } else {
      keys->push_back("0\t" + t[0]);
    }
  }
}

// Genotype counts of rows for --maf / --max-maf / --geno: per row the hom-REF / het / hom-ALT calls among the founders and the
// missing calls among all kept samples.  m_f / m_s: one bit pair (01) per founder / kept sample, 32 samples per word.
struct RowCounts {
  uint32_t ref2, het, alt2;  // founders
  uint32_t missing;          // kept samples
};
void count_rows(const uint8_t* rows, uint64_t stride, uint32_t n_rows, bool bed, uint32_t raw_sample_ct, const std::vector<uint64_t>& m_f,
                const std::vector<uint64_t>& m_s, RowCounts* out) {
  const uint64_t kLo = 0x5555555555555555ull;
  const uint64_t row_bytes = (static_cast<uint64_t>(raw_sample_ct) + 3) / 4;
  const size_t words = m_f.size();
  for (uint32_t r = 0; r < n_rows; ++r) {
    const uint8_t* row = rows + static_cast<uint64_t>(r) * stride;
    uint32_t c00 = 0, c01 = 0, c10 = 0, miss = 0;
    for (size_t w = 0; w < words; ++w) {
      uint64_t x = 0;
      const uint64_t left = row_bytes - 8 * w;
      memcpy(&x, row + 8 * w, (left < 8) ? left : 8);
      const uint64_t lo = x & kLo, hi = (x >> 1) & kLo;
      const uint64_t b00 = ~(lo | hi) & kLo, b01 = lo & ~hi, b10 = hi & ~lo, b11 = lo & hi;
      c00 += static_cast<uint32_t>(__builtin_popcountll(b00 & m_f[w]));
      c01 += static_cast<uint32_t>(__builtin_popcountll(b01 & m_f[w]));
      c10 += static_cast<uint32_t>(__builtin_popcountll(b10 & m_f[w]));
      miss += static_cast<uint32_t>(__builtin_popcountll((bed ? b01 : b11) & m_s[w]));
    }
    if (bed) {  // 00 hom-ALT, 01 missing, 10 het, 11 hom-REF (pgenlib_read.cc:2157)
      uint32_t c11 = 0;
      for (size_t w = 0; w < words; ++w) {
        uint64_t x = 0;
        const uint64_t left = row_bytes - 8 * w;
        memcpy(&x, row + 8 * w, (left < 8) ? left : 8);
        c11 += static_cast<uint32_t>(__builtin_popcountll(x & (x >> 1) & kLo & m_f[w]));
      }
      out[r] = {c11, c10, c00, miss};
    } else {    // 00 hom-REF, 01 het, 10 hom-ALT, 11 missing
      out[r] = {c00, c01, c10, miss};
    }
  }
}


// One multi-threaded pass over the rows of the variants `todo` (raw indices, ascending) -- what --geno / --maf and --mind count from before the
// variant list is final: fn(thread, rows, n, q) gets n rows, rec_bytes apart, of the variants todo[q .. q + n).  Fixed-width rows are read where
// they lie in the mapping; variable-width records are decoded in runs of file-consecutive variants (ldp_pgen_read, all host threads) first.
template <class F>
static void for_each_row_run(ldp_pgen* pg, const std::string& gpath, const uint8_t* direct_rows, uint64_t rec_bytes, const std::vector<uint32_t>& todo, uint32_t nthreads, F fn) {
  if (direct_rows) {
    std::atomic<size_t> next(0);
    const size_t kTask = 2048;
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < nthreads; ++t) {
      pool.emplace_back([&, t]() {
        for (size_t q0 = next.fetch_add(kTask); q0 < todo.size(); q0 = next.fetch_add(kTask)) {
          const size_t q1 = std::min(todo.size(), q0 + kTask);
          for (size_t q = q0; q < q1; ++q) {
            fn(t, direct_rows + static_cast<uint64_t>(todo[q]) * rec_bytes, 1u, q);
          }
        }
      });
    }
    for (std::thread& th : pool) {
      th.join();
    }
    return;
  }
  const uint32_t max_run = std::max<uint32_t>(1, static_cast<uint32_t>((256ull << 20) / std::max<uint64_t>(rec_bytes, 1)));
  std::vector<uint8_t> decoded;
  for (size_t q0 = 0; q0 < todo.size();) {
    uint32_t run = 1;
    while ((q0 + run < todo.size()) && (todo[q0 + run] == todo[q0] + run) && (run < max_run)) {
      ++run;
    }
    decoded.resize(static_cast<size_t>(run) * rec_bytes);
    if (ldp_pgen_read(pg, todo[q0], run, decoded.data(), rec_bytes, 0)) {
      die(6, "Error: %s: %s\n", gpath.c_str(), ldp_pgen_last_error(pg));
    }
    std::atomic<uint32_t> next(0);
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < nthreads; ++t) {
      pool.emplace_back([&, t]() {
        for (uint32_t r0 = next.fetch_add(256); r0 < run; r0 = next.fetch_add(256)) {
          fn(t, decoded.data() + static_cast<uint64_t>(r0) * rec_bytes, std::min(256u, run - r0), q0 + r0);
        }
      });
    }
    for (std::thread& th : pool) {
      th.join();
    }
    q0 += run;
  }
}

CountFilters::CountFilters(const Args& args, uint32_t kept_samples) : A(args) {
  geno_on = (A.geno != 1.0);
  mac_on = (A.min_allele_ddosage != 0) || (A.max_allele_ddosage != ~0ull);
  freq_on = (A.min_maf != 0.0) || (A.max_maf != 1.0) || mac_on;
  missing_max = static_cast<uint32_t>(static_cast<int32_t>(A.geno * (1 + kSmallEpsilon) * static_cast<double>(kept_samples)));
  min_maf = A.min_maf * (1.0 - kSmallEpsilon);
  max_maf = A.max_maf * (1.0 + kSmallEpsilon);
  // (a run of --hardy alone: the reference applies --geno, which the report depends on, and none of the filters behind the report)
  const bool consumer = A.have_prune || A.have_r2 || A.het || A.king;
  freq_on = freq_on && consumer;
  hwe_on = A.hwe && consumer;
  hwe_ln_base = A.hwe_ln_thresh * (1 + kSmallEpsilon);
  hwe_coeff = (A.hwe_sample_size_term <= 0) ? 0.0 : (A.hwe_sample_size_term * -2.3025850929940457);
}

bool CountFilters::drops(uint32_t missing, uint64_t ref2, uint64_t het, uint64_t alt2, const std::pair<uint64_t, uint64_t>* dosage, const double* hwe_ln_p) {
  if (geno_on && (missing > missing_max)) {
    ++geno_removed;
    return true;
  }
  if (hwe_on && hwe_ln_p) {
    // EnforceHweThresh (plink2_filter.cc:3604-3623, :3688-3695): nobody called = kept and not counted as an observation; keep-fewhet spares
    // a variant without het excess before any p-value is looked at
    const uint64_t obs = ref2 + het + alt2;
    if (obs && !(A.hwe_keep_fewhet && (het * het <= 4 * ref2 * alt2))) {
      hwe_min_obs = std::min(hwe_min_obs, static_cast<uint32_t>(obs));
      hwe_max_obs = std::max(hwe_max_obs, static_cast<uint32_t>(obs));
      if (*hwe_ln_p < hwe_ln_base + static_cast<double>(obs) * hwe_coeff) {
        ++hwe_removed;
        return true;
      }
    }
  }
  if (freq_on) {
    // allele counts in 16384ths of a copy: the hardcalls', or -- a record with dosages -- the founders' dosage sums
    uint64_t ref_ct = (2ull * ref2 + het) * 16384ull, alt_ct = (2ull * alt2 + het) * 16384ull;
    if (dosage) {
      ref_ct = dosage->first;
      alt_ct = dosage->second;
    }
    const uint64_t tot = ref_ct + alt_ct;
    if (mac_on) {
      // GetTypedDdosage, nonmajor mode, two alleles (plink2_filter.cc:3765-3767) on allele_ddosages = 2 x these sums
      // (plink2_data.cc:2441-2442)
      const uint64_t typed_dd = 2 * std::min(ref_ct, alt_ct);
      if ((typed_dd < A.min_allele_ddosage) || (typed_dd > A.max_allele_ddosage)) {
        ++freq_removed;
        return true;
      }
    }
    const double ref_freq = tot ? (static_cast<double>(ref_ct) * (1.0 / static_cast<double>(tot))) : 0.5;  // plink2_filter.cc:2137-2147
    const double nonref_freq = 1.0 - ref_freq;
    const double typed = (nonref_freq < ref_freq) ? nonref_freq : ref_freq;  // GetTypedFreq, nonmajor mode, two alleles (:3715-3723)
    if ((((A.min_maf != 0.0) || (A.max_maf != 1.0))) && (((A.min_maf != 0.0) && (typed < min_maf)) || ((A.max_maf < 1.0) && (typed > max_maf)))) {
      ++freq_removed;
      return true;
    }
  }
  return false;
}

void CountFilters::log_counts(const std::function<void()>& after_geno) const {
  if (geno_on) {
    logprintf("--geno: %u variant%s removed due to missing genotype data.\n", geno_removed, (geno_removed == 1) ? "" : "s");
  }
  if (after_geno) {
    after_geno();
  }
  if (hwe_on) {  // plink2_filter.cc:3697-3710
    const char* midp = A.hwe_midp ? " midp" : "";
    const char* fewhet = A.hwe_keep_fewhet ? " keep-fewhet" : "";
    if ((A.hwe_sample_size_term == -1) && (!A.hwe_keep_fewhet) && (static_cast<double>(hwe_max_obs) * 0.0005 * -2.3025850929940457 < hwe_ln_base)) {
      logprintf("Error: --hwe filter is suspiciously strict for the sample size; you may be\nfiltering out many variants with association signals.\n");
      logprintf_ww("If you are performing routine QC, consider using --hwe with a sample-size term (e.g. \"--hwe 1e-5 0.001%s\" results in a threshold of 1e-6 with 1000 observations, 1e-7 with 2000 observations, etc.), and/or specifying 'keep-fewhet' to remove only variants with heterozygosity excess.\n", midp);
      die(7, "Alternatively, if the strictness is intentional (e.g. you are preparing data\nfor a method that requires variants to be near Hardy-Weinberg equilibrium),\nexplicitly specify a sample-size term of 0.\n");
    } else if ((A.hwe_sample_size_term <= 0) && (static_cast<uint64_t>(hwe_max_obs) * 9 > static_cast<uint64_t>(hwe_min_obs) * 10)) {
      // ("10%.0 Consider": what the reference's own format string, which leaves its percent sign unescaped, prints through glibc)
      logprintf_ww("Warning: --hwe observation counts vary by more than 10%%.0 Consider using --hwe with a sample-size term (e.g. \"--hwe 1e-5 0.001%s%s\" results in a threshold of 1e-6 with 1000 observations, 1e-7 with 2000 observations, etc.), and/or filtering out high-missingness variants with --geno.\n", midp, fewhet);
    }
    logprintf_ww("--hwe%s%s: %u variant%s removed due to Hardy-Weinberg exact test (founders only).\n", midp, fewhet, hwe_removed, (hwe_removed == 1) ? "" : "s");
  }
  if (freq_on) {
    logprintf("%u variant%s removed due to allele frequency threshold(s)\n(--maf/--max-maf/--mac/--max-mac).\n", freq_removed, (freq_removed == 1) ? "" : "s");
  }
}

const char* device_filter_refusal(const Args& A, bool has_dosage, uint32_t kept_samples, uint32_t founder_ct) {
  if (g_dbg.host_filter) {
    return "--debug-host-filter";
  }
  if (((!A.have_prune) && (A.have_r2 || !(A.any_report() || A.het || A.hardy || A.king))) || A.pairphase) {  // (a run of reports, of --het, of --hardy or of --make-king-table alone loads like the prune)
    return A.pairphase ? "--indep-pairphase plans its engines before the load" : "the r^2 outputs and --clump plan their engines before the load";
  }
  if (A.gpus != 1) {
    return "more than one GPU (no engine holds every row)";
  }
  if (has_dosage) {
    return "the file has dosage tracks (frequencies come from the dosages)";
  }
  if (kept_samples != founder_ct) {
    return "non-founders among the kept samples (--geno counts them, the device's rows hold founders only)";
  }
  return nullptr;
}

// --extract / --exclude by ID (TokenExtractExclude, plink2_filter.cc:367: every variant carrying a listed ID, unknown IDs ignored)
VariantFilter::VariantFilter(const Args& args, const Variants& variants) : A(args), V(variants), by_chrom((!args.chr_keep.empty()) || (!args.chr_drop.empty()) || args.autosome) {
  for (const std::string& fn : A.extract_files) {
    for (std::string& t : tokens_of_file(fn)) {
      extract_ids_.insert(std::move(t));
    }
  }
  for (const std::string& fn : A.exclude_files) {
    for (std::string& t : tokens_of_file(fn)) {
      exclude_ids_.insert(std::move(t));
    }
  }
}

const ChromFacts& VariantFilter::chrom(const std::string& name) {
  if (last_ && (*last_name_ == name)) {
    return *last_;
  }
  auto it = chroms_.find(name);
  if (it == chroms_.end()) {
    ChromFacts c;
    c.code = chrom_code(name);
    c.out = by_chrom && (((!A.chr_keep.empty()) && !chrom_listed(A.chr_keep, name)) || ((!A.chr_drop.empty()) && chrom_listed(A.chr_drop, name)) ||
                         (A.autosome && !((c.code >= 1) && (c.code <= 22))));
    c.cls = chrom_class(name, A.allow_extra_chr, &c.zero);
    it = chroms_.emplace(name, c).first;
  }
  last_name_ = &it->first;
  last_ = &it->second;
  return *last_;
}

// One bit pair (01) per founder (m_f) / kept sample (m_s), 32 samples per word, and how many there are of each: as is_founder and sample_kept
// stand when it is asked for (--mind and --make-founders change them between the stages)
struct SampleMasks {
  std::vector<uint64_t> m_f, m_s;
  uint32_t kept_samples = 0, founders = 0;
};
static SampleMasks sample_masks(const Session& S) {
  const uint32_t raw_sample_ct = static_cast<uint32_t>(S.is_founder.size());
  SampleMasks M;
  M.m_f.assign((static_cast<size_t>(raw_sample_ct) + 31) / 32, 0);
  M.m_s = M.m_f;
  for (uint32_t sx = 0; sx < raw_sample_ct; ++sx) {
    const uint64_t bit = 1ull << (2 * (sx & 31));
    if (S.sample_kept.empty() || S.sample_kept[sx]) {
      M.m_s[sx >> 5] |= bit;
      ++M.kept_samples;
    }
    if (S.is_founder[sx]) {
      M.m_f[sx >> 5] |= bit;
      ++M.founders;
    }
  }
  return M;
}

static uint32_t host_pass_threads() {
  return std::max(1u, std::min(64u, std::thread::hardware_concurrency()));
}

// the autosomal variants of the final list (chromosome 0 counts as one, CountNonAutosomalVariants plink2_common.cc:3334); returns how many are not
static uint32_t autosomal_of_final_list(const Session& S, std::vector<uint32_t>* todo) {
  uint32_t non_autosomal = 0;
  for (size_t k = 0; k < S.inc.size(); ++k) {
    if (S.vcls[k] >= 3) {
      ++non_autosomal;
    } else {
      todo->push_back(S.inc[k]);
    }
  }
  return non_autosomal;
}

// ---- --mind (LoadSampleMissingCts plink2_data.cc:10846-10990, MindFilter plink2_filter.cc:3329-3383)
// per-sample missing hardcalls of rows: cts[sample of the file] += 1 for every kept sample (m_s: one 01 bit pair per kept sample) whose call is missing
static void count_sample_missing(const uint8_t* rows, uint64_t stride, uint32_t n_rows, bool bed, uint32_t raw_sample_ct, const std::vector<uint64_t>& m_s, uint32_t* cts) {
  const uint64_t kLo = 0x5555555555555555ull;
  const uint64_t row_bytes = (static_cast<uint64_t>(raw_sample_ct) + 3) / 4;
  const size_t words = m_s.size();
  for (uint32_t r = 0; r < n_rows; ++r) {
    const uint8_t* row = rows + static_cast<uint64_t>(r) * stride;
    for (size_t w = 0; w < words; ++w) {
      uint64_t x = 0;
      const uint64_t left = row_bytes - 8 * w;
      memcpy(&x, row + 8 * w, (left < 8) ? left : 8);
      // .pgen: 11 is missing; .bed: 01 (pgenlib_read.cc:2157)
      uint64_t miss = (bed ? (x & ~(x >> 1)) : (x & (x >> 1))) & kLo & m_s[w];
      while (miss) {
        ++cts[32 * w + (static_cast<uint32_t>(__builtin_ctzll(miss)) >> 1)];
        miss &= miss - 1;
      }
    }
  }
}

// ... on the threads of a pass over the rows: one array per thread, summed at the end
struct SampleMissingParts {
  std::vector<std::vector<uint32_t>> part;
  SampleMissingParts(uint32_t nthreads, size_t mask_words) : part(nthreads, std::vector<uint32_t>(32 * mask_words, 0)) {}
  std::vector<uint32_t> sum(uint32_t raw_sample_ct) const {
    std::vector<uint32_t> cts(raw_sample_ct, 0);
    for (const std::vector<uint32_t>& p : part) {
      for (uint32_t sx = 0; sx < raw_sample_ct; ++sx) {
        cts[sx] += p[sx];
      }
    }
    return cts;
  }
};
// per sample of the file: the missing hardcalls of the kept samples over the variants `todo`
static std::vector<uint32_t> sample_missing_over(const Session& S, const std::vector<uint32_t>& todo, const std::vector<uint64_t>& m_s) {
  const uint32_t raw_sample_ct = static_cast<uint32_t>(S.is_founder.size());
  int storage_mode = 0;
  ldp_pgen_info(S.pg, nullptr, nullptr, &storage_mode, nullptr, nullptr);
  const bool bed = (storage_mode == 0x01);
  uint64_t rec_bytes = (static_cast<uint64_t>(raw_sample_ct) + 3) / 4;
  const uint8_t* direct_rows = static_cast<const uint8_t*>(ldp_pgen_direct_rows(S.pg, &rec_bytes));  // NULL for variable-width
  const uint32_t nthreads = host_pass_threads();
  SampleMissingParts parts(nthreads, m_s.size());
  for_each_row_run(S.pg, S.gpath, direct_rows, rec_bytes, todo, nthreads, [&](uint32_t t, const uint8_t* rows, uint32_t n, size_t) {
    count_sample_missing(rows, rec_bytes, n, bed, raw_sample_ct, m_s, parts.part[t].data());
  });
  return parts.sum(raw_sample_ct);
}

uint32_t mind_decide(const Session& S,const std::vector<uint32_t>& missing_cts, std::vector<uint8_t>* removed) {
  const Args& A = S.A;
  const uint32_t raw_sample_ct = static_cast<uint32_t>(S.is_founder.size());
  // a sample goes when it misses more than (int32_t)(variant_ct * (thresh * (1 + 2^-44))) calls (MindFilter :3340-3342; no chrY here)
  const double thresh = A.mind * (1 + kSmallEpsilon);
  const uint32_t max_missing = static_cast<uint32_t>(static_cast<int32_t>(static_cast<double>(S.mind_variant_ct) * thresh));
  removed->assign(raw_sample_ct, 0);
  uint32_t removed_ct = 0;
  for (uint32_t sx = 0; sx < raw_sample_ct; ++sx) {
    if ((S.sample_kept.empty() || S.sample_kept[sx]) && (missing_cts[sx] > max_missing)) {
      (*removed)[sx] = 1;
      ++removed_ct;
    }
  }
  logprintf("%u sample%s removed due to missing genotype data (--mind).\n", removed_ct, (removed_ct == 1) ? "" : "s");
  if (removed_ct) {
    // WriteSampleIds, plink2_common.cc:4219-4270
    const std::string path = A.out + ".mindrem.id";
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) {
      die(3, "Error: Failed to open %s for writing.\n", path.c_str());
    }
    fputs(S.fid_present ? "#FID\tIID" : "#IID", f);
    fputs(S.sample_sids.empty() ? "\n" : "\tSID\n", f);
    for (uint32_t sx = 0; sx < raw_sample_ct; ++sx) {
      if ((*removed)[sx]) {
        fputs(S.sample_keys[sx].c_str() + (S.fid_present ? 0 : 2), f);  // (no FID column: every key starts with "0<tab>")
        if (!S.sample_sids.empty()) {
          fputc('\t', f);
          fputs(S.sample_sids[sx].c_str(), f);
        }
        fputc('\n', f);
      }
    }
    if (fclose(f)) {
      die(5, "Error: File write failure: %s.\n", path.c_str());
    }
    logprintf("ID%s written to %s .\n", (removed_ct == 1) ? "" : "s", path.c_str());
  }
  return removed_ct;
}

void mind_apply(Session& S, const std::vector<uint8_t>& removed) {
  if (S.sample_kept.empty()) {
    S.sample_kept.assign(S.is_founder.size(), 1);
  }
  bool any = false;
  for (size_t sx = 0; sx < removed.size(); ++sx) {
    if (removed[sx]) {
      S.sample_kept[sx] = 0;
      S.is_founder[sx] = 0;
    }
    any = any || S.sample_kept[sx];
  }
  if (!any) {  // plink2.cc:1836-1838
    die(13, "Error: No samples remaining after main filters.\n");
  }
}

// The --mind stage of load_inputs(): the variants the table filters leave (--chr / --not-chr / --autosome, --extract / --exclude, --snps-only,
// --max-alleles; chromosome 0 and multiallelic variants count, everything before --geno does), then one of
//   * a restarted run: the first run's decision, applied as --remove would have;
//   * the decision left to run_prune() (S.mind_device), which reads the counts off the resident image;
//   * the host pass: a multi-threaded pass over the rows like the one --geno has -- fixed-width rows where they lie, variable-width records through
//     ldp_pgen_read, .bed codes -- that counts the missing hardcalls of every kept sample (a dosage track changes no hardcall), then the decision.
static void sample_filter_mind(Session& S, VariantFilter& filter) {
  const Args& A = S.A;
  const Variants& V = S.V;
  std::vector<uint32_t> todo;
  bool any_x_mt = false, any_multiallelic = false;
  filter.walk(
      [&](const std::string& cur, const ChromFacts& c) {
        if (c.out) {
          return;
        }
        if (c.cls == 2) {
          die(6, "Error: Invalid chromosome code '%s'. (Use --allow-extra-chr to force it to be accepted.)\n", cur.c_str());
        }
        if (c.cls == 4) {
          // (the reference counts chrY over the males only and gives the others a smaller denominator, MindFilter :3341-3355: not built)
          die(63, "Error: --mind with chrY variants ('%s') is not supported by plink2-hip: filter them out (--autosome, --not-chr y) or pre-filter with plink2.\n", cur.c_str());
        }
        any_x_mt = any_x_mt || (c.cls == 3) || (c.cls == 5);
      },
      [&](uint32_t v, const ChromFacts&) {
        any_multiallelic = any_multiallelic || (V.alt_ct[v] > 1);
        todo.push_back(v);
      });
  S.mind_variant_ct = static_cast<uint32_t>(todo.size());
  if (S.mind_decided) {
    mind_apply(S, S.mind_removed);
  }
  const SampleMasks M = sample_masks(S);
  if (S.mind_decided) {
    g_log_mute = false;
    logprintf("--mind: %u sample%s remaining (%u founder%s); the rows are loaded again without the removed samples.\n", M.kept_samples, (M.kept_samples == 1) ? "" : "s", M.founders,
              (M.founders == 1) ? "" : "s");
    g_log_mute = true;
    return;
  }
  // from the resident image where the variant filters may come from the device's records, and where in addition the image's rows ARE the
  // hardcalls of the variants counted and its columns the final founders
  const char* reason = device_filter_refusal(A, ldp_pgen_has_dosage(S.pg) != 0, M.kept_samples, M.founders);
  if (!reason) {
    reason = A.dry_run ? "--dry-run"
             : ((A.make_founders && !A.make_founders_first) ? "--make-founders runs after --mind, on the samples it leaves"
             : (any_x_mt ? "chrX / MT variants (their rows are built for engines of their own)"
             : (any_multiallelic ? "multiallelic variants (their rows are collapsed on the way into the image)" : nullptr)));
  }
  if (A.dry_run) {
    logprintf("dry-run: sample filter (--mind): host pass over %u variant%s\n", S.mind_variant_ct, (S.mind_variant_ct == 1) ? "" : "s");
  }
  if (!reason) {
    S.mind_device = true;
    return;
  }
  const double t0 = now_s();
  const std::vector<uint32_t> missing_cts = sample_missing_over(S, todo, M.m_s);
  std::vector<uint8_t> removed;
  if (mind_decide(S, missing_cts, &removed)) {
    mind_apply(S, removed);
  }
  if (A.timing) {
    logprintf("[timing] sample filter (--mind): host pass (%.3f s; %s)\n", now_s() - t0, reason);
  }
}

// The reports' stage of load_inputs(): what they list, then either the decision that run_prune() writes them from the engine's records
// (S.report_device: the same conditions as for the count filters, device_filter_refusal) or the host's pass -- count_rows over a founder mask
// and a kept-sample mask, the per-sample pass --mind has, ldp_pgen_read_alleles for a variant with several ALT alleles -- and the writer.
static void reports_stage(Session& S, VariantFilter& filter) {
  const Args& A = S.A;
  const uint32_t raw_sample_ct = static_cast<uint32_t>(S.is_founder.size());
  reports_list_variants(S, filter, &S.report_variants);
  const std::vector<uint32_t>& todo = S.report_variants;
  if (todo.empty()) {  // plink2.cc:2484-2487 (kPglRetDegenerateData)
    die(13, "Error: No variants remaining after main filters.\n");
  }
  const SampleMasks M = sample_masks(S);
  const std::vector<uint64_t>&m_f = M.m_f, &m_s = M.m_s;
  const uint32_t kept_samples = M.kept_samples, founders = M.founders;
  if (A.rep_freq && A.rep_freq_counts && (kept_samples != founders) && !A.ac_founders) {  // plink2.cc:2102-2105
    die(7, "Error: --mac/--max-mac/\"--freq counts\" specified, but with neither\n--ac-founders nor --nonfounders; and nonfounders are present.\n");
  }
  const char* reason = device_filter_refusal(A, false, kept_samples, founders);
  if (!reason) {
    reason = A.dry_run ? "--dry-run"
             : ((founders < 2) ? "fewer than two founders (no engine)"
             : ((A.rep_smiss() && (founders > ldp_matrix_pipe_max_founders())) ? "more founders than the resident 2-bit image takes (the per-sample counts are read off it)" : nullptr));
  }
  if (A.dry_run) {
    logprintf("dry-run: reports: %s%s\n", reason ? "host pass: " : "from the device's count pass", reason ? reason : "");
  }
  if (!reason) {
    S.report_device = true;
    return;
  }
  S.report_host_reason = reason;
  const double t0 = now_s();
  const bool bed = (S.storage_mode == 0x01);
  const uint64_t rec_bytes = S.rec_bytes;
  const uint32_t nthreads = host_pass_threads();
  const bool two_sets = (kept_samples != founders) && A.rep_gcount;  // (--geno-counts counts every kept sample, --freq the founders)
  std::vector<RowCounts> fc(todo.size()), sc(two_sets ? todo.size() : 0);
  SampleMissingParts parts(A.rep_smiss() ? nthreads : 0, m_s.size());
  for_each_row_run(S.pg, S.gpath, S.direct_rows, rec_bytes, todo, nthreads, [&](uint32_t t, const uint8_t* rows, uint32_t n, size_t q) {
    count_rows(rows, rec_bytes, n, bed, raw_sample_ct, m_f, m_s, &fc[q]);
    if (two_sets) {
      count_rows(rows, rec_bytes, n, bed, raw_sample_ct, m_s, m_s, &sc[q]);
    }
    if (!parts.part.empty()) {
      count_sample_missing(rows, rec_bytes, n, bed, raw_sample_ct, m_s, parts.part[t].data());
    }
  });
  ReportCounts C;
  C.variants = todo;
  C.kept_sample_ct = kept_samples;
  C.missing.resize(todo.size());
  C.f_ref2.resize(todo.size());
  C.f_het.resize(todo.size());
  C.f_alt2.resize(todo.size());
  for (size_t q = 0; q < todo.size(); ++q) {
    C.missing[q] = fc[q].missing;
    C.f_ref2[q] = fc[q].ref2;
    C.f_het[q] = fc[q].het;
    C.f_alt2[q] = fc[q].alt2;
  }
  if (two_sets) {
    C.s_ref2.resize(todo.size());
    C.s_het.resize(todo.size());
    C.s_alt2.resize(todo.size());
    for (size_t q = 0; q < todo.size(); ++q) {
      C.s_ref2[q] = sc[q].ref2;
      C.s_het[q] = sc[q].het;
      C.s_alt2[q] = sc[q].alt2;
    }
  }
  if (A.rep_freq) {
    std::vector<uint8_t> lo, hi;
    for (size_t q = 0; q < todo.size(); ++q) {
      if (S.V.alt_ct[todo[q]] > 1) {
        reports_count_alleles_host(S, todo[q], &lo, &hi, &C.allele_cts[static_cast<uint32_t>(q)]);
      }
    }
  }
  C.sample_missing = parts.sum(raw_sample_ct);
  const bool muted = g_log_mute;  // (a run that --mind started over logs nothing twice; these lines are this load's own)
  g_log_mute = false;
  write_reports(S, C);
  g_log_mute = muted;
  if (A.timing) {
    logprintf("[timing] reports: host pass (%.3f s; %s)\n", now_s() - t0, reason);
  }
}

// What het_stage and king_stage ask about the variants the table filters leave, and their refusal of chromosome 0 beside a command that strips
// it (the reference counts unplaced variants as autosomal; the prune and the windowed tables strip them from the one list kept here).
// command / alone: "--het" / "--het", "--make-king-table" / "it"
struct ImageRowScan {
  bool any_non_autosomal = false, any_multiallelic = false;
};
static ImageRowScan scan_for_image_pass(const Session& S, VariantFilter& filter, const char* command, const char* alone) {
  const Args& A = S.A;
  const Variants& V = S.V;
  ImageRowScan scan;
  filter.walk([](const std::string&, const ChromFacts&) {},
              [&](uint32_t v, const ChromFacts& c) {
                if (c.zero && (A.have_prune || (A.r2_table && !A.r2_inter))) {
                  die(63, "Error: %s beside %s with chromosome 0 variants ('%s') is not supported by plink2-hip: run %s on its own, or filter them out (--not-chr 0).\n", command,
                      A.have_prune ? "the prune" : "a windowed r^2 command", V.id[v].c_str(), alone);
                }
                scan.any_non_autosomal = scan.any_non_autosomal || (c.cls >= 3);
                scan.any_multiallelic = scan.any_multiallelic || (V.alt_ct[v] > 1);
              });
  return scan;
}
// ... and the end of their reasons for the host's pass; too_many_founders: the command's own wording of it
static const char* image_pass_refusal(uint32_t founders, const char* too_many_founders, const ImageRowScan& scan) {
  return (founders < 2) ? "fewer than two founders (no engine)"
         : ((founders > ldp_matrix_pipe_max_founders()) ? too_many_founders
         : (scan.any_non_autosomal ? "chrX / chrY / MT variants (their rows are built for engines of their own)"
         : (scan.any_multiallelic ? "multiallelic variants (their rows are collapsed on the way into the image)" : nullptr)));
}

// The --het stage of load_inputs(): what is refused, then where the sums come from -- the resident image after the filters (S.het_device: the
// conditions of the count filters, device_filter_refusal, and rows that ARE the hardcalls of autosomal biallelic variants), or het_host_pass().
static void het_stage(Session& S, VariantFilter& filter) {
  const Args& A = S.A;
  if (ldp_pgen_has_dosage(S.pg)) {
    // (the reference takes the allele frequencies from the dosages where a record has them, plink2_data.cc:2421-2443)
    die(63, "Error: %s holds dosage data, which --het of plink2-hip does not read.  Use plink2 --make-pgen erase-dosage first.\n", S.gpath.c_str());
  }
  const ImageRowScan scan = scan_for_image_pass(S, filter, "--het", "--het");
  const SampleMasks M = sample_masks(S);
  const char* reason = device_filter_refusal(A, false, M.kept_samples, M.founders);
  if (!reason) {
    reason = A.dry_run ? "--dry-run" : image_pass_refusal(M.founders, "more founders than the resident 2-bit image takes (the per-sample sums are read off it)", scan);
  }
  if (A.dry_run) {
    logprintf("dry-run: --het: %s%s\n", reason ? "host pass: " : "from the resident image", reason ? reason : "");
  }
  S.het_device = !reason;
  S.het_host_reason = reason;
}

void het_host_pass(Session& S) {
  const Args& A = S.A;
  const Variants& V = S.V;
  const double t0 = now_s();
  const uint32_t raw_sample_ct = static_cast<uint32_t>(S.is_founder.size());
  std::vector<uint32_t> todo;
  const uint32_t non_autosomal = autosomal_of_final_list(S, &todo);
  het_preamble(S, static_cast<uint32_t>(todo.size()), non_autosomal);
  const SampleMasks M = sample_masks(S);
  const std::vector<uint64_t>&m_f = M.m_f, &m_s = M.m_s;
  const size_t words = m_s.size();
  const uint32_t kept_samples = M.kept_samples;
  const bool bed = (S.storage_mode == 0x01);
  const uint64_t rec_bytes = S.rec_bytes;
  const uint32_t nthreads = host_pass_threads();
  // first pass: the founders' allele counts, hence every variant's expected heterozygosity and the plan of the integer sums
  std::vector<RowCounts> fc(todo.size());
  for_each_row_run(S.pg, S.gpath, S.direct_rows, rec_bytes, todo, nthreads, [&](uint32_t, const uint8_t* rows, uint32_t n, size_t q) {
    count_rows(rows, rec_bytes, n, bed, raw_sample_ct, m_f, m_s, &fc[q]);
  });
  std::vector<double> ehet(todo.size(), 0.0);
  std::vector<uint8_t> ok(todo.size(), 0);
  std::vector<uint8_t> lo, hi;
  std::vector<uint32_t> cts;
  for (size_t q = 0; q < todo.size(); ++q) {
    if (V.alt_ct[todo[q]] > 1) {
      reports_count_alleles_host(S, todo[q], &lo, &hi, &cts);
    } else {
      cts.assign({2 * fc[q].ref2 + fc[q].het, 2 * fc[q].alt2 + fc[q].het});
    }
    ok[q] = het_expected(cts.data(), static_cast<uint32_t>(cts.size()), A.het_small_sample, &ehet[q]) ? 1 : 0;
    if (ok[q] && (!S.direct_rows) && (V.alt_ct[todo[q]] <= 1) && (fc[q].missing == kept_samples)) {
      ok[q] = 0;  // (het_all_missing_skipped, p2h_cli.h)
    }
  }
  HetPlan plan;
  plan.build(ehet, ok);
  // second pass: per kept sample the het calls, the missing calls and the q_v of the missing calls, over the kept variants
  const uint64_t kLo = 0x5555555555555555ull;
  const uint64_t row_bytes = (static_cast<uint64_t>(raw_sample_ct) + 3) / 4;
  std::vector<HetSums> part(nthreads);
  for (HetSums& p : part) {
    p.het_ct.assign(32 * words, 0);
    p.missing_ct.assign(32 * words, 0);
    p.missing_weight.assign(32 * words, 0);
  }
  for_each_row_run(S.pg, S.gpath, S.direct_rows, rec_bytes, todo, nthreads, [&](uint32_t t, const uint8_t* rows, uint32_t n, size_t q) {
    HetSums& p = part[t];
    for (uint32_t r = 0; r < n; ++r) {
      if ((!plan.include[q + r]) || (V.alt_ct[todo[q + r]] > 1)) {
        continue;
      }
      const uint8_t* row = rows + static_cast<uint64_t>(r) * rec_bytes;
      const uint64_t wt = plan.weight[q + r];
      for (size_t w = 0; w < words; ++w) {
        uint64_t x = 0;
        const uint64_t left = row_bytes - 8 * w;
        memcpy(&x, row + 8 * w, (left < 8) ? left : 8);
        const uint64_t b_lo = x & kLo, b_hi = (x >> 1) & kLo;
        // .pgen: 01 het, 11 missing; .bed: 10 het, 01 missing (pgenlib_read.cc:2157)
        uint64_t het = (bed ? (b_hi & ~b_lo) : (b_lo & ~b_hi)) & m_s[w];
        uint64_t miss = (bed ? (b_lo & ~b_hi) : (b_lo & b_hi)) & m_s[w];
        while (het) {
          ++p.het_ct[32 * w + (static_cast<uint32_t>(__builtin_ctzll(het)) >> 1)];
          het &= het - 1;
        }
        while (miss) {
          const uint32_t sx = static_cast<uint32_t>(32 * w) + (static_cast<uint32_t>(__builtin_ctzll(miss)) >> 1);
          ++p.missing_ct[sx];
          p.missing_weight[sx] += wt;
          miss &= miss - 1;
        }
      }
    }
  });
  HetSums sums;
  sums.het_ct.assign(raw_sample_ct, 0);
  sums.missing_ct.assign(raw_sample_ct, 0);
  sums.missing_weight.assign(raw_sample_ct, 0);
  for (const HetSums& p : part) {
    for (uint32_t sx = 0; sx < raw_sample_ct; ++sx) {
      sums.het_ct[sx] += p.het_ct[sx];
      sums.missing_ct[sx] += p.missing_ct[sx];
      sums.missing_weight[sx] += p.missing_weight[sx];
    }
  }
  // a variant with several ALT alleles: every call with two different alleles is a het one (HetThread :10063-10079), from the reader's allele pairs
  for (size_t q = 0; q < todo.size(); ++q) {
    if (plan.include[q] && (V.alt_ct[todo[q]] > 1)) {
      reports_count_alleles_host(S, todo[q], &lo, &hi, &cts);
      for (uint32_t sx = 0; sx < raw_sample_ct; ++sx) {
        if ((!S.sample_kept.empty()) && !S.sample_kept[sx]) {
          continue;
        }
        if (lo[sx] == 255) {
          ++sums.missing_ct[sx];
          sums.missing_weight[sx] += plan.weight[q];
        } else if (lo[sx] != hi[sx]) {
          ++sums.het_ct[sx];
        }
      }
    }
  }
  het_write(S, plan, sums);
  if (A.timing) {
    logprintf("[timing] --het: host pass (%.3f s; %s)\n", now_s() - t0, S.het_host_reason ? S.het_host_reason : "the r^2 outputs and --clump plan their engines before the load");
  }
}

// The --make-king-table stage of load_inputs(), het_stage's neighbour: where the pair counts come from -- the resident image after the filters
// (S.king_device: the conditions of het_device), or king_host_pass().  The table is made of hardcalls, so a dosage file is no refusal: it
// takes the host's pass.
static void king_stage(Session& S, VariantFilter& filter) {
  const Args& A = S.A;
  const ImageRowScan scan = scan_for_image_pass(S, filter, "--make-king-table", "it");
  const SampleMasks M = sample_masks(S);
  const char* reason = device_filter_refusal(A, false, M.founders, M.founders);
  if (!reason) {
    reason = (M.kept_samples != M.founders) ? "non-founders among the kept samples (the table lists them, the device's rows hold founders only)"
             : (ldp_pgen_has_dosage(S.pg) ? "the file has dosage tracks" : nullptr);
  }
  if (!reason) {
    reason = image_pass_refusal(M.founders, "more founders than the resident 2-bit image takes (the pair counts are read off it)", scan);
  }
  if (A.dry_run) {
    char num[40];
    *format_g6(A.king_filter, num) = '\0';
    logprintf("dry-run: --make-king-table: cols 0x%x%s%s, filter %s; %s%s\n", A.king_cols, A.king_counts ? ", counts" : "", A.king_zs ? ", zs" : "", A.king_filter_given ? num : "none",
              reason ? "host pass: " : "from the resident image", reason ? reason : "");
  }
  S.king_device = (!reason) && !A.dry_run;  // (a dry run prints the decision and touches no device)
  S.king_host_reason = reason ? reason : "--dry-run";
}

void king_host_pass(Session& S) {
  const Args& A = S.A;
  const double t0 = now_s();
  const uint32_t raw_sample_ct = static_cast<uint32_t>(S.is_founder.size());
  std::vector<uint32_t> todo;
  const uint32_t non_autosomal = autosomal_of_final_list(S, &todo);
  std::vector<uint32_t> kept;  // sample of the file per kept sample
  for (uint32_t sx = 0; sx < raw_sample_ct; ++sx) {
    if (S.sample_kept.empty() || S.sample_kept[sx]) {
      kept.push_back(sx);
    }
  }
  const uint32_t sample_ct = static_cast<uint32_t>(kept.size());
  king_preamble(S, sample_ct, static_cast<uint32_t>(todo.size()), non_autosomal);
  // sample-major bit-planes over the variants of the list: het, hom, hom-ALT (.bed: hom-A1).  Two threads may hold variants of the same word.
  const size_t words = (todo.size() + 63) / 64;
  std::vector<uint64_t> het(static_cast<size_t>(sample_ct) * words, 0), hom(het.size(), 0), alt(het.size(), 0);
  const bool bed = (S.storage_mode == 0x01);
  const uint64_t rec_bytes = S.rec_bytes;
  const uint32_t nthreads = host_pass_threads();
  for_each_row_run(S.pg, S.gpath, S.direct_rows, rec_bytes, todo, nthreads, [&](uint32_t, const uint8_t* rows, uint32_t n, size_t q) {
    for (uint32_t r = 0; r < n; ++r) {
      const uint8_t* row = rows + static_cast<uint64_t>(r) * rec_bytes;
      const size_t w = (q + r) >> 6;
      const uint64_t bit = 1ull << ((q + r) & 63);
      for (uint32_t s = 0; s < sample_ct; ++s) {
        const uint32_t c = code_at(row, kept[s]);
        // .pgen: 00 hom-REF, 01 het, 10 hom-ALT, 11 missing; .bed: 00 hom-A1, 01 missing, 10 het, 11 hom-A2 (pgenlib_read.cc:2157)
        const bool is_het = bed ? (c == 2) : (c == 1);
        const bool is_hom = bed ? ((c == 0) || (c == 3)) : ((c == 0) || (c == 2));
        const bool is_alt = bed ? (c == 0) : (c == 2);
        if (is_het) {
          __atomic_fetch_or(&het[static_cast<size_t>(s) * words + w], bit, __ATOMIC_RELAXED);
        } else if (is_hom) {
          __atomic_fetch_or(&hom[static_cast<size_t>(s) * words + w], bit, __ATOMIC_RELAXED);
          if (is_alt) {
            __atomic_fetch_or(&alt[static_cast<size_t>(s) * words + w], bit, __ATOMIC_RELAXED);
          }
        }
      }
    }
  });
  const double t1 = now_s();
  KingWriter w(S);
  king_pairs_host(het, hom, alt, words, sample_ct, nthreads, &w);
  w.finish(static_cast<uint32_t>(todo.size()));
  if (A.timing) {
    logprintf("[timing] --make-king-table: host pass (%u samples, %zu variants; bit-planes %.3f s, pairs and writing %.3f s; %s)\n", sample_ct, todo.size(), t1 - t0, now_s() - t1,
              S.king_host_reason ? S.king_host_reason : "the r^2 outputs and --clump plan their engines before the load");
  }
}

// --make-founders (MakeFounders, plink2_filter.cc:4372-4443): a non-founder with a parent (both, with 'require-2-missing') that
// is not among the samples in play becomes a founder; 'first' applies it before --keep / --remove, else after them
static void make_founders(Session& S, const std::vector<std::pair<std::string, std::string>>& parent_keys, const std::vector<uint8_t>* included) {
  const Args& A = S.A;
  const std::vector<std::string>& sample_keys = S.sample_keys;
  std::unordered_set<std::string> present;
  bool any_nonfounder = false;
  for (size_t sx = 0; sx < sample_keys.size(); ++sx) {
    if ((!included) || (*included)[sx]) {
      present.insert(sample_keys[sx]);
      any_nonfounder = any_nonfounder || !S.is_founder[sx];
    }
  }
  if (!any_nonfounder) {
    logprintf("Note: Skipping --make-founders since there are no nonfounders.\n");
    return;
  }
  uint32_t affected = 0;
  for (size_t sx = 0; sx < sample_keys.size(); ++sx) {
    if (S.is_founder[sx] || (included && !(*included)[sx])) {
      continue;
    }
    const uint32_t missing = (present.count(parent_keys[sx].first) ? 0u : 1u) + (present.count(parent_keys[sx].second) ? 0u : 1u);
    if (missing > (A.make_founders_require2 ? 1u : 0u)) {
      S.is_founder[sx] = 1;
      ++affected;
    }
  }
  logprintf("--make-founders: %u sample%s affected.\n", affected, (affected == 1) ? "" : "s");
}

// --keep, then --remove (KeepOrRemove, plink2_filter.cc:1227-1261; plink2.cc)
static void keep_remove_samples(Session& S) {
  const Args& A = S.A;
  std::vector<uint8_t> in(S.is_founder.size(), 1);
  for (int pass = 0; pass < 2; ++pass) {
    const std::vector<std::string>& files = pass ? A.remove_files : A.keep_files;
    if (files.empty()) {
      continue;
    }
    const char* flag = pass ? "remove" : "keep";
    std::vector<std::string> keys;
    for (const std::string& fn : files) {
      load_sample_id_list(fn, flag, &keys);
    }
    std::unordered_set<std::string> listed;
    size_t dups = 0;
    for (std::string& k : keys) {
      dups += listed.insert(std::move(k)).second ? 0 : 1;
    }
    uint32_t remaining = 0;
    for (size_t sx = 0; sx < in.size(); ++sx) {
      const bool hit = listed.count(S.sample_keys[sx]) != 0;
      in[sx] = static_cast<uint8_t>(in[sx] && (pass ? !hit : hit));
      remaining += in[sx];
    }
    logprintf("--%s: %u sample%s remaining.\n", flag, remaining, (remaining == 1) ? "" : "s");
    if (dups) {
      logprintf("Warning: At least %zu duplicate ID%s in --%s file(s).\n", dups, (dups == 1) ? "" : "s", flag);
    }
  }
  for (size_t sx = 0; sx < in.size(); ++sx) {
    S.is_founder[sx] = static_cast<uint8_t>(S.is_founder[sx] && in[sx]);
  }
  S.sample_kept = in;
  if (std::find(in.begin(), in.end(), 1) == in.end()) {  // plink2.cc:1836-1838
    die(13, "Error: No samples remaining after main filters.\n");
  }
}

// The samples' stage of load_inputs(): the sample file, --make-founders first, --keep / --remove.  parent_keys: what a later --make-founders needs
static void load_sample_tables(Session& S, std::vector<std::pair<std::string, std::string>>* parent_keys) {
  const Args& A = S.A;
  const bool sample_filter = (!A.keep_files.empty()) || (!A.remove_files.empty());
  const bool want_keys = sample_filter || A.make_founders || (A.mind < 1.0) || A.rep_smiss() || A.het || A.king;
  load_samples(A, &S.is_founder, &S.sex, want_keys ? &S.sample_keys : nullptr, A.make_founders ? parent_keys : nullptr, &S.fid_present, &S.sample_sids);
  if (A.make_founders && A.make_founders_first) {
    make_founders(S, *parent_keys, nullptr);
  }
  if (sample_filter) {
    keep_remove_samples(S);
  }
}

// the genotype file (.bed / fixed-width .pgen / standard variable-width .pgen): --mind needs it earlier than the other stages
static void open_genotypes(Session& S) {
  if (S.pg) {
    return;
  }
  const Args& A = S.A;
  S.is_bed = !A.bed.empty();
  S.gpath = S.is_bed ? A.bed : A.pgen;
  if (ldp_pgen_open_indexed(S.gpath.c_str(), A.pgi.empty() ? nullptr : A.pgi.c_str(), static_cast<uint32_t>(S.is_founder.size()), static_cast<uint32_t>(S.V.id.size()), &S.pg)) {
    die(6, "Error: %s: %s\n", S.gpath.c_str(), ldp_pgen_last_error(S.pg));
  }
}

// The early checks of load_inputs(): the tables' log lines, the founder counts the commands need, the genotype file and what its dosages refuse
static void early_checks(Session& S) {
  const Args& A = S.A;
  S.raw_sample_ct = static_cast<uint32_t>(S.is_founder.size());
  const uint32_t raw_sample_ct = S.raw_sample_ct;
  const SampleMasks M = sample_masks(S);
  S.founder_ct += M.founders;
  const uint32_t founder_ct = S.founder_ct;
  logprintf("%u sample%s loaded from %s (%u founder%s).\n", raw_sample_ct, raw_sample_ct == 1 ? "" : "s",
            (A.psam.empty() ? A.fam : A.psam).c_str(), founder_ct, founder_ct == 1 ? "" : "s");
  S.raw_variant_ct = static_cast<uint32_t>(S.V.id.size());
  logprintf("%u variant%s loaded from %s.\n", S.raw_variant_ct, S.raw_variant_ct == 1 ? "" : "s", (A.pvar.empty() ? A.bim : A.pvar).c_str());

  if (A.have_prune && founder_ct < 50 && !A.bad_ld) {  // plink2.cc:2063-2071
    if (raw_sample_ct < 50) {
      die(13, "Error: This run estimates linkage disequilibrium between variants, but there\nare less than 50 samples to estimate from.  You should perform this operation\non a larger dataset.\n(Strictly speaking, you can also override this error with --bad-ld, but this is\nalmost always a bad idea.)\n");
    }
    die(13, "Error: This run estimates linkage disequilibrium between variants, but there\nare less than 50 founders to estimate from.  --make-founders may help.\n(Strictly speaking, you can also override this error with --bad-ld, but this is\nalmost always a bad idea.)\n");
  }
  if (A.het && (!A.het_small_sample) && !A.bad_freqs) {  // plink2.cc:2073-2088: --het needs decent allele frequencies (no --read-freq, no --nonfounders here)
    const uint32_t sample_ct = M.kept_samples;
    if ((sample_ct >= 50) && (founder_ct < 50)) {
      die(13, "Error: This run requires decent allele frequencies, but they aren't being\nloaded with --read-freq, and less than 50 founders are available to impute them\nfrom.  Possible solutions:\n* You can use --nonfounders to include nonfounders when imputing allele\n  frequencies.\n* You can generate (with --freq) or obtain an allele frequency file based on a\n  larger similar-population reference dataset, and load it with --read-freq.\n* (Not recommended) You can override this error with --bad-freqs.\n");
    }
    if (sample_ct < 50) {
      die(13, "Error: This run requires decent allele frequencies, but they aren't being\nloaded with --read-freq, and less than 50 samples are available to impute them\nfrom.\nYou should generate (with --freq) or obtain an allele frequency file based on a\nlarger similar-population reference dataset, and load it with --read-freq.\n%s",
          (sample_ct != founder_ct) ? "If you're certain you want to proceed without doing that, use --bad-freqs to\noverride this error, and consider using --nonfounders as well.\n" : "");
    }
  }
  if ((founder_ct < 2) && (A.have_prune || A.have_r2)) {
    die(7, "Error: %s requires at least two founders. (--make-founders may come in handy here.)\n", A.have_prune ? (A.pairphase ? "--indep-pairphase" : "--indep-pairwise") : "--r2-unphased");
  }

  open_genotypes(S);
  ldp_pgen_info(S.pg, nullptr, nullptr, &S.storage_mode, &S.encoding, &S.has_multiallelic);
  S.has_dosage = ldp_pgen_has_dosage(S.pg) != 0;
  if (S.has_dosage) {
    // The reference takes allele frequencies from the dosages when a file has them (plink2_data.cc:2421-2443).  For
    // --indep-pairwise that is the major allele's frequency in the tie-break -- r^2 itself is computed from the hardcalls
    // (plink2_ld.cc:699-723) --, which run_prune() reproduces (ldp_pgen_dosage_sums); --maf / --max-maf compare the same
    // frequencies.  Everything else that would read dosages (the r^2 of --r2-unphased / --clump, phased dosages) is refused
    // rather than computed from hardcalls.
    const char* what = A.have_r2 ? "--r2-unphased / --clump" : (A.pairphase ? "--indep-pairphase" : nullptr);
    if (what) {
      ldp_pgen_close(S.pg);
      die(63, "Error: %s holds dosage data, which plink2-hip reads for --indep-pairwise only (%s would be\ncomputed from hardcalls, unlike plink2).  Use plink2 --make-pgen erase-dosage first.\n", S.gpath.c_str(), what);
    }
  }
  S.rec_bytes = (static_cast<uint64_t>(raw_sample_ct) + 3) / 4;
  S.direct_rows = static_cast<const uint8_t*>(ldp_pgen_direct_rows(S.pg, &S.rec_bytes));  // NULL for variable-width
}

// The count filters' stage of load_inputs().  --geno / --maf / --max-maf / --mac / --hwe (and --hardy's report) need genotype counts before the
// variant list is final: where the job allows it the variants are loaded first and the filters decided from the engine's records (S.device_filter;
// run_prune: ldp_get_variant_recs + ldp_restrict_variants); otherwise one multi-threaded pass over the rows of the variants the table filters
// leave (host popcounts; the rows are read again when they go to the device).  Returns, for the host's pass, 1 per raw variant it drops.
static std::vector<uint8_t> count_filter_stage(Session& S, VariantFilter& filter) {
  const Args& A = S.A;
  const Variants& V = S.V;
  const bool freq_filter = (A.min_maf != 0.0) || (A.max_maf != 1.0) || (A.min_allele_ddosage != 0) || (A.max_allele_ddosage != ~0ull);
  const bool hwe_any = A.hwe || A.hardy;
  std::vector<uint8_t> drop_by_counts;
  if (!((freq_filter || (A.geno != 1.0) || hwe_any) && (A.have_prune || A.have_r2 || A.het || A.hardy || A.king))) {
    return drop_by_counts;
  }
  std::vector<uint32_t> todo;
  std::vector<uint8_t> todo_haploid;  // chrY / MT (--hwe / --hardy alone: neither tested nor listed)
  uint32_t haploid_ct = 0;
  filter.walk(
      [&](const std::string& cur, const ChromFacts& c) {
        if ((!c.out) && (c.cls >= 3) && (freq_filter || (A.geno != 1.0))) {
          die(63, "Error: --maf / --max-maf / --mac / --max-mac / --geno on chrX, chrY or MT ('%s') are not supported by plink2-hip: filter them out (--autosome, --chr) or pre-filter with plink2.\n", cur.c_str());
        }
      },
      [&](uint32_t v, const ChromFacts& c) {
        if (c.cls == 3) {  // (.hardy.x and the joint test of females' genotypes and males' alleles are not built)
          die(63, "Error: --hwe / --hardy with a chrX variant ('%s') are not supported by plink2-hip: filter chrX out (--autosome, --not-chr) or use plink2.\n", V.id[v].c_str());
        }
        if (V.alt_ct[v] > 1) {
          if (hwe_any) {  // (one test per allele against the rest, on genotype counts nobody makes here)
            die(63, "Error: --hwe / --hardy with a multiallelic variant ('%s') are not supported by plink2-hip: --max-alleles 2 leaves them out.\n", V.id[v].c_str());
          }
          die(63, "Error: --maf / --max-maf / --mac / --max-mac / --geno with multiallelic variants ('%s') are not supported by plink2-hip.\n", V.id[v].c_str());
        }
        todo.push_back(v);
        todo_haploid.push_back((c.cls > 3) ? 1 : 0);
        haploid_ct += (c.cls > 3) ? 1u : 0u;
      });
  const SampleMasks M = sample_masks(S);
  // (--dry-run plans on the final variant list without a device: it takes the host's pass and says which one a run would take.)
  S.count_filters = true;
  S.kept_sample_ct = M.kept_samples;
  S.host_filter_reason = device_filter_refusal(A, S.has_dosage, M.kept_samples, S.founder_ct);
  if ((!S.host_filter_reason) && haploid_ct) {
    S.host_filter_reason = "chrY / MT variants among the kept ones (--hwe / --hardy leave them alone; the device's pass takes autosomes only)";
  }
  if (A.dry_run) {
    logprintf("dry-run: variant filters: %s%s\n", S.host_filter_reason ? "host pass: " : "from the device's count pass", S.host_filter_reason ? S.host_filter_reason : "");
  }
  S.device_filter = (!S.host_filter_reason) && !A.dry_run;
  if (S.device_filter) {
    return drop_by_counts;
  }
  const double t_filter0 = now_s();
  std::vector<RowCounts> counts(todo.size());
  const bool bed = (S.storage_mode == 0x01);
  const uint32_t nthreads = host_pass_threads();
  for_each_row_run(S.pg, S.gpath, S.direct_rows, S.rec_bytes, todo, nthreads, [&](uint32_t, const uint8_t* rows, uint32_t n, size_t q) {
    count_rows(rows, S.rec_bytes, n, bed, S.raw_sample_ct, M.m_f, M.m_s, &counts[q]);
  });
  if (S.has_dosage && freq_filter) {
    std::vector<uint32_t> with_track;
    for (uint32_t v : todo) {
      if (ldp_pgen_variant_has_dosage(S.pg, v)) {
        with_track.push_back(v);
      }
    }
    S.need_dosage_sums(with_track);
  }
  drop_by_counts.assign(S.raw_variant_ct, 0);
  CountFilters F(A, M.kept_samples);
  // --hwe / --hardy: ln p of every diploid variant --geno leaves, from the founders' counts, on the reader's threads (ldp_hwe_ln_p_host:
  // hwe_kernel's arithmetic on the CPU); one set of values serves both where their `midp` settings agree
  std::vector<double> ln_hwe, ln_hardy;
  if (hwe_any) {
    const double t_hwe0 = now_s();
    const bool two = A.hwe && A.hardy && (A.hwe_midp != A.hardy_midp);
    const int midp_first = A.hwe ? (A.hwe_midp ? 1 : 0) : (A.hardy_midp ? 1 : 0);
    ln_hwe.assign(todo.size(), 0.0);
    if (two) {
      ln_hardy.assign(todo.size(), 0.0);
    }
    std::vector<uint8_t> tie(todo.size(), 0);
    std::atomic<size_t> next(0);
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < nthreads; ++t) {
      pool.emplace_back([&]() {
        for (size_t q0 = next.fetch_add(64); q0 < todo.size(); q0 = next.fetch_add(64)) {
          for (size_t q = q0; q < std::min(todo.size(), q0 + 64); ++q) {
            const RowCounts& c = counts[q];
            if (todo_haploid[q] || F.fails_geno(c.missing)) {
              continue;
            }
            uint8_t fl = 0, fl2 = 0;
            ln_hwe[q] = ldp_hwe_ln_p_host(static_cast<uint32_t>(c.ref2), static_cast<uint32_t>(c.het), static_cast<uint32_t>(c.alt2), midp_first, &fl);
            if (two) {
              ln_hardy[q] = ldp_hwe_ln_p_host(static_cast<uint32_t>(c.ref2), static_cast<uint32_t>(c.het), static_cast<uint32_t>(c.alt2), A.hardy_midp ? 1 : 0, &fl2);
            }
            tie[q] = static_cast<uint8_t>(1 | (((fl | fl2) & 1) << 1));
          }
        }
      });
    }
    for (std::thread& th : pool) {
      th.join();
    }
    for (uint8_t x : tie) {
      S.hwe_host_ct += x & 1;
      S.hwe_host_ties += x >> 1;
    }
    S.hwe_host_s = now_s() - t_hwe0;
    if (A.timing) {  // (here, not with the pass's own timing: --hwe's strictness error ends the run before that)
      logprintf("[timing] --hwe / --hardy: host pass (%u p-values from ldp_hwe_ln_p_host on %u threads, %.3f s; %u with a tolerance tie)\n", S.hwe_host_ct, nthreads, S.hwe_host_s,
                S.hwe_host_ties);
    }
  }
  HardyCounts H;
  H.haploid_skipped = haploid_ct;
  for (size_t q = 0; q < todo.size(); ++q) {
    const RowCounts& c = counts[q];
    if (A.hardy && (!todo_haploid[q]) && !F.fails_geno(c.missing)) {
      H.add(todo[q], static_cast<uint32_t>(c.ref2), static_cast<uint32_t>(c.het), static_cast<uint32_t>(c.alt2), ln_hardy.empty() ? ln_hwe[q] : ln_hardy[q]);
    }
    // (a record with dosages: the founders' dosage sums instead of the hardcalls' allele counts)
    const auto dd = S.dosage_sums.find(todo[q]);
    if (F.drops(c.missing, c.ref2, c.het, c.alt2, (dd != S.dosage_sums.end()) ? &dd->second : nullptr, (hwe_any && !todo_haploid[q]) ? &ln_hwe[q] : nullptr)) {
      drop_by_counts[todo[q]] = 1;
    }
  }
  F.log_counts([&]() {
    if (A.hardy) {
      write_hardy(S, H);
    }
  });
  S.host_filter_s = now_s() - t_filter0;
  if (A.timing) {
    logprintf("[timing] variant filters: host pass (%.3f s; %s)\n", S.host_filter_s, S.host_filter_reason ? S.host_filter_reason : "--dry-run");
  }
  return drop_by_counts;
}

// The final variant list of load_inputs(): what the table filters and the host's count filters (drop_by_counts; empty: none) leave, with the
// chromosome order index, chromosome 0 stripped where the reference strips it, and the checks on the whole list (split chromosomes, filters
// that leave nothing, sortedness)
static void final_variant_list(Session& S, VariantFilter& filter, const std::vector<uint8_t>& drop_by_counts) {
  const Args& A = S.A;
  const Variants& V = S.V;
  const uint32_t raw_variant_ct = S.raw_variant_ct;
  const char* table_path = (A.pvar.empty() ? A.bim : A.pvar).c_str();
  std::vector<uint32_t>&inc = S.inc, &chr_idx = S.chr_idx, &bps = S.bps;
  uint32_t skipped = 0, after_extract = 0, after_exclude = 0;
  std::unordered_set<std::string> seen_chr;
  const ChromFacts* cur = nullptr;
  uint32_t fo = 0;
  inc.reserve(raw_variant_ct);
  chr_idx.reserve(raw_variant_ct);
  bps.reserve(raw_variant_ct);
  for (uint32_t v = 0; v < raw_variant_ct; ++v) {
    if ((!cur) || (V.chrom[v] != V.chrom[v - 1])) {
      if (!seen_chr.insert(V.chrom[v]).second) {
        die(6, "Error: %s has a split chromosome. Use --make-pgen + --sort-vars to remedy this.\n", table_path);
      }
      fo += cur ? 1 : 0;
      cur = &filter.chrom(V.chrom[v]);
    }
    const VariantFilter::Verdict verdict = filter.verdict(v);
    if (verdict == VariantFilter::kByTable) {
      continue;
    }
    after_extract += (verdict != VariantFilter::kByExtract) ? 1 : 0;
    after_exclude += (verdict == VariantFilter::kPass) ? 1 : 0;
    if ((verdict != VariantFilter::kPass) || ((!drop_by_counts.empty()) && drop_by_counts[v])) {
      continue;
    }
    if (cur->zero && (A.have_prune || (A.r2_table && !A.r2_inter))) {  // (the all-pairs modes keep chromosome 0)
      if (!S.device_filter) {
        ++skipped;
        continue;
      }
      // (the count filters see chromosome 0 too, and only what they leave of it is "ignored": such variants are loaded and filtered with
      // the others, and run_prune() drops and reports the survivors)
      S.inc_chr0.resize(inc.size() + 1, 0);
      S.inc_chr0.back() = 1;
    }
    if (cur->cls == 2) {
      die(6, "Error: Invalid chromosome code '%s'. (Use --allow-extra-chr to force it to be accepted.)\n", V.chrom[v].c_str());
    }
    S.vcls.push_back(static_cast<uint8_t>(cur->cls));
    inc.push_back(v);
    chr_idx.push_back(fo);
    bps.push_back(V.bp[v]);
  }
  if (!A.extract_files.empty()) {
    logprintf("--extract: %u variant%s remaining.\n", after_extract, (after_extract == 1) ? "" : "s");
  }
  if (!A.exclude_files.empty()) {
    logprintf("--exclude: %u variant%s remaining.\n", after_exclude, (after_exclude == 1) ? "" : "s");
  }
  // filters applied while the variant table loads (--autosome / --chr / --not-chr / --max-alleles) that leave nothing:
  // plink2.cc:1025-1050, kPglRetInconsistentInput, flag names in kLoadFilterLogFlagnames order
  const bool table_filter = filter.by_chrom || (A.max_alleles != 0xffffffffu) || A.snps_only;
  if (table_filter && raw_variant_ct) {
    bool any_loaded = false;
    for (uint32_t v = 0; (v < raw_variant_ct) && !any_loaded; ++v) {
      any_loaded = filter.table_passes(v);
    }
    if (!any_loaded) {
      std::string flags;
      for (const char* nm : {A.autosome ? "autosome" : "", A.chr_keep.empty() ? "" : "chr", A.chr_drop.empty() ? "" : "not-chr",
                             (A.max_alleles != 0xffffffffu) ? "max-alleles" : "", A.snps_only ? "snps-only" : ""}) {
        if (*nm) {
          flags += (flags.empty() ? "--" : " + --");
          flags += nm;
        }
      }
      die(7, "Error: All %u variant%s in %s excluded by %s.\n", raw_variant_ct, (raw_variant_ct == 1) ? "" : "s", table_path, flags.c_str());
    }
  }
  const bool any_main_filter = table_filter || (!A.extract_files.empty()) || (!A.exclude_files.empty()) || (!drop_by_counts.empty()) || S.device_filter;
  if (any_main_filter && inc.empty() && (!skipped)) {  // plink2.cc:2484-2487 (kPglRetDegenerateData)
    die(13, "Error: No variants remaining after main filters.\n");
  }
  if (skipped) {
    logprintf("--%s: Ignoring %u chromosome 0 variant%s.\n", A.have_prune ? (A.pairphase ? "indep-pairphase" : "indep-pairwise") : (A.have_clump ? "clump" : "r2-unphased"), skipped, skipped == 1 ? "" : "s");
  }
  S.variant_ct = static_cast<uint32_t>(inc.size());
  if ((A.window_is_bp || A.r2_table) && !S.device_filter) {  // (device_filter: the check is about the variants the count filters leave, run_prune())
    for (uint32_t k = 1; k < S.variant_ct; ++k) {
      if (chr_idx[k] == chr_idx[k - 1] && bps[k] < bps[k - 1]) {
        if (A.have_prune) {  // plink2.cc:2926-2929
          die(6, "Error: When the window size is in kb units, LD-based pruning requires a sorted\n.pvar/.bim.  Retry this command after using --make-pgen/--make-bed +\n--sort-vars to sort your data.\n");
        }
        if (A.have_clump) {  // plink2.cc:2998-3001
          die(7, "Error: --clump requires a sorted .pvar/.bim.  Retry this command after using\n--make-pgen/--make-bed + --sort-vars to sort your data.\n");
        }
        die(6, "Error: --r[2]-[un]phased runs require a sorted .pvar/.bim.  Retry this command\nafter using --make-pgen/--make-bed + --sort-vars to sort your data.\n");  // plink2.cc:2944-2947
      }
    }
  }
}

// chrX and chrY variants run on engines of their own (different sample sets); MT stays with the autosomes --
// except under --indep-pairphase, where the autosomes carry two haplotypes per founder and MT one
// (IndepPairphaseUpdateSubcontig, plink2_ld.cc:1491-1511)
static void split_into_engines(Session& S) {
  for (uint32_t k = 0; k < S.variant_ct; ++k) {
    (S.vcls[k] == 3 ? S.xk : (S.vcls[k] == 4 ? S.yk : ((S.vcls[k] == 5 && S.A.pairphase) ? S.tk : S.mk))).push_back(k);
  }
  S.m_ct = static_cast<uint32_t>(S.mk.size());
  S.m_chr.resize(S.m_ct);
  S.m_bps.resize(S.m_ct);
  for (uint32_t q = 0; q < S.m_ct; ++q) {
    S.m_chr[q] = S.chr_idx[S.mk[q]];
    S.m_bps[q] = S.bps[S.mk[q]];
  }
}

void load_inputs(Session& S, int argc, char** argv) {
  S.t_begin = S.t_begin_first ? S.t_begin_first : now_s();
  S.A = parse_args(argc, argv);
  const Args& A = S.A;
  if (!g_log) {
    g_log = fopen((A.out + ".log").c_str(), "w");
  }
  // (a run that --mind started over: this load's lines were logged by the first one, up to the one line below that says what changed)
  g_log_mute = S.mind_decided;
  logprintf("plink2-hip: MI355X-native --indep-pairwise (drop-in for that path of PLINK v2.0)\n");
  logprintf("Options in effect:\n ");
  for (int i = 1; i < argc; ++i) {
    logprintf(" %s", argv[i]);
  }
  logprintf("\n\n");

  // the variant table parses on its own thread and the HIP runtime initialises on another while the
  // sample file is read
  std::thread t_variants([&S]() { load_variants(S.A, &S.V); });
  // (the HIP runtime start-up AND the context of device 0 -- its queues, the first pinned allocation -- beside the table parsing)
  S.t_joined = now_s();   // (a restarted run: the runtime is up, there is nothing to start or to join)
  if (!S.mind_decided) {
    S.t_hip = std::thread([&S]() { const double t0 = now_s(); if (ldp_device_count() > 0) { (void)ldp_prewarm(0); } S.t_hip_init = now_s() - t0; });
  }
  std::vector<std::pair<std::string, std::string>> parent_keys;
  load_sample_tables(S, &parent_keys);
  // ---- --mind: after --keep / --remove, before --make-founders (unless 'first'), --geno and the founder count (plink2.cc:1600-1840).  It needs
  // the genotype file and the variant-table filter -- the --extract / --exclude ID sets -- earlier than the other stages, and they where they always were
  std::optional<VariantFilter> filter;
  if (A.mind < 1.0) {  // plink2.cc:8910
    t_variants.join();
    open_genotypes(S);
    filter.emplace(A, S.V);
    sample_filter_mind(S, *filter);
  }
  if (A.make_founders && !A.make_founders_first) {
    make_founders(S, parent_keys, S.sample_kept.empty() ? nullptr : &S.sample_kept);
  }
  if (t_variants.joinable()) {
    t_variants.join();
  }
  S.t_parse = now_s() - S.t_begin;
  early_checks(S);

  // ---- variant filters: --chr / --not-chr / --autosome by chromosome, --max-alleles, --snps-only, then --extract, then --exclude by ID
  if (!filter) {
    filter.emplace(A, S.V);
  }
  if (((A.min_allele_ddosage != 0) || (A.max_allele_ddosage != ~0ull)) && (!A.ac_founders) && (sample_masks(S).kept_samples != S.founder_ct)) {
    // (plink2.cc:2102-2105; plink2-hip counts alleles over the founders: the --nonfounders alternative is not offered)
    die(7, "Error: --mac/--max-mac/\"--freq counts\" specified, but with neither\n--ac-founders nor --nonfounders; and nonfounders are present.\n");
  }
  // ---- the count reports: after the sample filters, before --geno / --maf / --mac (plink2.cc:2370-2470)
  if (A.any_report()) {
    reports_stage(S, *filter);
  }
  // (a run of reports alone: nothing reads the filtered variant list, and the reference applies no variant filter then)
  if (A.het) {
    het_stage(S, *filter);
  }
  if (A.king) {
    king_stage(S, *filter);
  }
  const std::vector<uint8_t> drop_by_counts = count_filter_stage(S, *filter);
  if ((S.report_device || S.mind_device || S.het_device || S.king_device) && !S.device_filter) {
    // (no count filter, or none that reached the device: the rows the reports, --mind, --het or --make-king-table read off the image are loaded under the
    // all-pairs plan all the same, chromosome 0 included; run_prune() writes what they write and plans over what is left afterwards)
    S.device_filter = true;
    S.kept_sample_ct = S.founder_ct;
  }
  // ---- variant table: strip chromosome 0, chromosome order index, sortedness
  final_variant_list(S, *filter, drop_by_counts);
  split_into_engines(S);
  g_log_mute = false;
  if (A.het && A.have_r2) {
    // (the r^2 outputs and --clump keep the host's filters: the variant list is final here.  Beside the prune, or alone, run_prune() calls the
    // pass once its list is -- after the device's filters, after a --mind decided there)
    het_host_pass(S);
  }
  if (A.king && A.have_r2 && !A.dry_run) {
    king_host_pass(S);
  }
}


}  // namespace p2h
