// p2h_r2_job.h -- plink2-hip: what the writers of the r^2 outputs share (p2h_r2.cpp: the unphased matrices and tables; p2h_r2_phased.cpp:
// the --r2-phased / --r-phased table): the job run_r2() sets up, the .vcor table's column set, the chromosome names of its lines
#ifndef P2H_R2_JOB_H
#define P2H_R2_JOB_H
#include "p2h_cli.h"

namespace p2h {

std::vector<uint8_t> vcor_row_variants(const Args& A, const Variants& V, const std::vector<uint32_t>& inc, uint32_t variant_ct, double thresh);

// names as the reference prints them (chrtoa with the default --output-chr: bare numbers, XY/PAR1/PAR2, contig names)
inline std::string vcor_chrom_name(const std::string& raw) {
    std::string name = raw;
    if (name.size() > 3 && (name[0] | 32) == 'c' && (name[1] | 32) == 'h' && (name[2] | 32) == 'r') {
      bool zero = false;
      const std::string rest = name.substr(3);
      bool numeric = !rest.empty();
      for (char c : rest) {
        numeric = numeric && (c >= '0' && c <= '9');
      }
      if (numeric || ieq(rest.c_str(), "XY") || ieq(rest.c_str(), "PAR1") || ieq(rest.c_str(), "PAR2")) {
        name = rest;
      }
      (void)zero;
    }
    bool numeric = !name.empty();
    for (char c : name) {
      numeric = numeric && (c >= '0' && c <= '9');
    }
    if (numeric) {
      const long v = strtol(name.c_str(), nullptr, 10);
      return (v == 25) ? std::string("XY") : std::to_string(v);
    }
    if (ieq(name.c_str(), "XY")) return std::string("XY");
    if (ieq(name.c_str(), "PAR1")) return std::string("PAR1");
    if (ieq(name.c_str(), "PAR2")) return std::string("PAR2");
    return name;
  }

// What the two writers of the r^2 outputs share (run_r2 sets it up: engine planned and fed, sex chromosomes prepared)
struct R2Job {
  Session& S;
  ldp_engine* e = nullptr;
  uint32_t shard_first = 0, shard_end = 0;  // --parallel k n: this piece's rows
  std::string piece_suffix, base;
  std::vector<uint8_t> is_x;                // per engine row: a chrX variant whose pairs take the male-weighted sums
  bool any_x = false;
  XWeighted xw;
  std::unordered_map<uint32_t, std::pair<uint32_t, double>> multi_maj;  // multiallelic variant -> (major allele, its frequency)
  std::vector<uint8_t> x_maj_alt;           // chrX-aware major allele (MAJ / NONMAJ columns)
  std::vector<double> x_maj_freq;
  explicit R2Job(Session& s) : S(s) {}
  // the entries of dense rows [r0, r0 + rows) x columns [c0, c0 + cols) (second variant j = row, first variant i = column,
  // i < j) that involve chrX, recomputed in place
  void x_fix_dense(void* buf, bool as_float, uint32_t r0, uint32_t rows, uint32_t c0, uint32_t cols, uint64_t ld) const {
    if (!any_x) {
      return;
    }
    if (g_dbg.x_host) {  // (test hook --debug-x-host: pair lists through ldp_pair_stats and the host arithmetic, as the band writers do)
      std::vector<uint32_t> fi, se;
      std::vector<double> vals;
      for (uint32_t q = 0; q < rows; ++q) {
        const uint32_t j = r0 + q;
        for (uint32_t i = c0; i < std::min(j, c0 + cols); ++i) {
          if (is_x[i] || is_x[j]) {
            fi.push_back(i);
            se.push_back(j);
          }
        }
      }
      xw.pairs(fi, se, &vals);
      for (size_t q = 0; q < fi.size(); ++q) {
        const uint64_t idx = static_cast<uint64_t>(se[q] - r0) * ld + (fi[q] - c0);
        if (as_float) {
          static_cast<float*>(buf)[idx] = static_cast<float>(vals[q]);
        } else {
          static_cast<double*>(buf)[idx] = vals[q];
        }
      }
      return;
    }
    // both engines' tuples of the block's chrX rows / columns from the pair kernels, combined on the device (ldp_r2_unphased_block_x)
    if (ldp_r2_unphased_block_x(xw.all, xw.male, xw.is_x.data(), xw.flip_all.empty() ? nullptr : xw.flip_all.data(), xw.flip_male.empty() ? nullptr : xw.flip_male.data(),
                                r0, rows, c0, cols, as_float ? 1 : 0, xw.unsquared ? 1 : 0, buf, ld)) {
      die(16, "Error: %s\n", ldp_last_error(xw.all));
    }
  }
};

// The column set of the .vcor table (VcorTable :11250-11390, VcorTableWriteThread :10836-10960): what each variant prints
// in front of the r^2, and the header line.
struct VcorColumns {
  const R2Job& J;
  const Args& A;
  const Variants& V;
  const std::vector<uint32_t>& inc;
  const std::vector<uint32_t>& bps;
  uint32_t cols = 0;
  std::vector<uint8_t> prov_bits;
  bool prov_all = false, provref_col = false;
  std::vector<uint8_t> maj_allele;
  std::vector<double> nonmaj_freq;
  explicit VcorColumns(const R2Job& job) : J(job), A(job.S.A), V(job.S.V), inc(job.S.inc), bps(job.S.bps) {
    ldp_engine* const e = J.e;
    ldp_pgen* const pg = J.S.pg;
    const uint32_t variant_ct = J.S.variant_ct, raw_variant_ct = J.S.raw_variant_ct;
    const std::vector<uint8_t>& is_x = J.is_x;
    const auto& multi_maj = J.multi_maj;
    const std::vector<uint8_t>& x_maj_alt = J.x_maj_alt;
    const std::vector<double>& x_maj_freq = J.x_maj_freq;
    cols = A.r2_cols;
    if (cols & kVcorColRef) {  // ProvrefCol (plink2_common.h:1549): 'provref' always, 'maybeprovref' when some included variant is flagged
      prov_bits.assign((static_cast<size_t>(raw_variant_ct) + 7) / 8, 0);
      int storage = ldp_pgen_provisional_ref(pg, prov_bits.data(), prov_bits.size());
      if ((storage == 0) && V.info_pr_header) {  // the .pgen leaves it to the .pvar's INFO/PR
        storage = 3;
        std::copy(V.info_pr.begin(), V.info_pr.begin() + std::min(V.info_pr.size(), prov_bits.size()), prov_bits.begin());
      }
      prov_all = (storage == 2);
      if (cols & kVcorColProvref) {
        provref_col = true;
      } else if (cols & kVcorColMaybeprovref) {
        provref_col = prov_all;
        for (uint32_t k = 0; (storage == 3) && (!provref_col) && (k < variant_ct); ++k) {
          provref_col = (prov_bits[inc[k] >> 3] >> (inc[k] & 7)) & 1;
        }
      }
    }
    // major allele and non-major frequency per variant (the allele-frequency pass: plink2_filter.cc:2137-2147, GetMajIdx)
    if (cols & (kVcorColMaj | kVcorColNonmaj | kVcorColFreq)) {
      std::vector<ldp_variant_rec> recs(variant_ct);
      if (variant_ct && ldp_get_variant_recs(e, 0, variant_ct, recs.data())) {
        die(16, "Error: %s\n", ldp_last_error(e));
      }
      maj_allele.assign(variant_ct, 0);
      nonmaj_freq.assign(variant_ct, 0.0);
      for (uint32_t k = 0; k < variant_ct; ++k) {
        const auto it = multi_maj.find(k);
        double maj_freq;
        if (it != multi_maj.end()) {  // (several ALT alleles, on chrX too: the allele-frequency pass's own major allele)
          maj_allele[k] = static_cast<uint8_t>(it->second.first);
          maj_freq = it->second.second;
        } else if (is_x[k]) {
          maj_allele[k] = x_maj_alt[k];
          maj_freq = x_maj_freq[k];
        } else {
          const uint64_t ref_ct = 2ull * recs[k].n_homref + recs[k].n_het, alt_ct = 2ull * recs[k].n_homalt + recs[k].n_het, tot = ref_ct + alt_ct;
          double ref_freq = 0.5;
          if (tot) {
            ref_freq = static_cast<double>(ref_ct) * (1.0 / static_cast<double>(tot));
          }
          maj_allele[k] = (ref_freq >= 0.5) ? 0 : 1;
          maj_freq = maj_allele[k] ? (1.0 - ref_freq) : ref_freq;  // GetAlleleFreq: the last allele's frequency is 1 - the others
        }
        nonmaj_freq[k] = 1.0 - maj_freq;
      }
    }
    // one variant's columns, each followed by a tab
  }
  void allele_text(uint32_t k, uint32_t allele, std::string* out) const {
    const uint32_t v = inc[k];
    if (!allele) {
      *out += V.ref[v];
      return;
    }
    const std::string& alt = V.alt[v];
    size_t p0 = 0;
    for (uint32_t a = 1; a < allele; ++a) {
      p0 = alt.find(',', p0) + 1;
    }
    out->append(alt, p0, std::min(alt.find(',', p0), alt.size()) - p0);
  }
  // one variant's columns, each followed by a tab
  void put(uint32_t k, const std::string& chr_name, std::string* out) const {
    char num[40];
    if (cols & kVcorColChrom) {
      *out += chr_name;
      *out += '\t';
    }
    if (cols & kVcorColPos) {
      *out += std::to_string(bps[k]);
      *out += '\t';
    }
    if (cols & kVcorColId) {
      *out += V.id[inc[k]];
      *out += '\t';
    }
    if (cols & kVcorColRef) {
      *out += V.ref[inc[k]];
      *out += '\t';
    }
    if (cols & kVcorColAlt1) {
      allele_text(k, 1, out);
      *out += '\t';
    }
    if (cols & kVcorColAlt) {
      *out += V.alt[inc[k]];
      *out += '\t';
    }
    if (provref_col) {
      *out += (prov_all || ((!prov_bits.empty()) && ((prov_bits[inc[k] >> 3] >> (inc[k] & 7)) & 1))) ? 'Y' : 'N';
      *out += '\t';
    }
    if (cols & kVcorColMaj) {
      allele_text(k, maj_allele[k], out);
      *out += '\t';
    }
    if (cols & kVcorColNonmaj) {
      const uint32_t allele_ct = static_cast<uint32_t>(V.alt_ct[inc[k]]) + 1;
      for (uint32_t a = 0; a < allele_ct; ++a) {
        if (a != maj_allele[k]) {
          allele_text(k, a, out);
          *out += ',';
        }
      }
      out->back() = '\t';
    }
    if (cols & kVcorColFreq) {
      out->append(num, format_g6(nonmaj_freq[k], num) - num);
      *out += '\t';
    }
  }
  std::string header() const {
  std::string hdr = "#";
  for (const char side : {'A', 'B'}) {
    const std::pair<uint32_t, const char*> names[] = {{kVcorColChrom, "CHROM_"}, {kVcorColPos, "POS_"}, {kVcorColId, "ID_"}, {kVcorColRef, "REF_"},
                                                      {kVcorColAlt1, "ALT1_"}, {kVcorColAlt, "ALT_"}, {0, "PROVISIONAL_REF_"}, {kVcorColMaj, "MAJ_"},
                                                      {kVcorColNonmaj, "NONMAJ_"}, {kVcorColFreq, "NONMAJ_FREQ_"}};
    for (const auto& nm : names) {
      if (nm.first ? ((cols & nm.first) != 0) : provref_col) {
        hdr += nm.second;
        hdr += side;
        if (!nm.first) {
          hdr += '?';
        }
        hdr += '\t';
      }
    }
  }
  if (A.r2_phased) {  // (VcorTable :11330-11345: the value, then D, then D' -- the absolute one where both were asked for)
    hdr += A.r_unsquared ? "PHASED_R" : "PHASED_R2";
    if (cols & kVcorColD) {
      hdr += "\tD";
    }
    if (cols & kVcorColDprimeAbs) {
      hdr += "\tABS_DPRIME";
    } else if (cols & kVcorColDprime) {
      hdr += "\tDPRIME";
    }
    hdr += '\n';
    return hdr;
  }
  hdr += A.r_unsquared ? "UNPHASED_R\n" : "UNPHASED_R2\n";
    return hdr;
  }
};

struct R2Job;
// p2h_r2_phased.cpp: the windowed --r2-phased / --r-phased table; phase = the engine of the phase-code rows, or nullptr
int write_vcor_table_phased(R2Job& J, ldp_engine* phase);
void refuse_unsupported_phased(const Session& S);
ldp_engine* build_phase_engine(Session& S, const ldp_params& RP, const std::vector<double>& cms);

}  // namespace p2h
#endif
