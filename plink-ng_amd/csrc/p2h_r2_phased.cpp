// p2h_r2_phased.cpp -- plink2-hip: the windowed --r2-phased / --r-phased table (one translation unit of the front-end; plink2_hip_cli.cpp has the overview)
//
// VcorTable (plink2_ld.cc:11025) with phased_calc: one line per pair A < B inside the window whose haplotype-frequency r^2 (or |r|)
// passes --ld-window-r2, with D and D' on request.  run_r2() (p2h_r2.cpp) has planned and fed the genotype engine as for the unphased
// table; this unit adds the phase-code rows of files with a hardcall-phase track (a second engine on the same plan), takes the five
// integers of the pairs that can pass from ldp_r2_phased_band_hits(), computes the statistic on the host (ldp_phased_ld) and applies the
// exact test there.  Column set, band / window logic, --ld-snp rows and the output writer are the unphased table's.
#include "p2h_r2_job.h"

namespace p2h {

// What this front-end does not take (exit 63, nothing computed).  Matrix shapes, inter-chr, --parallel and --gpus are refused while the
// flags are read (p2h_args.cpp); what depends on the data is refused here, before any device is touched.
void refuse_unsupported_phased(const Session& S) {
  const Args& A = S.A;
  const char* fl = A.r_unsquared ? "--r-phased" : "--r2-phased";
  for (uint32_t k = 0; k < S.variant_ct; ++k) {
    if (S.vcls[k] >= 3) {
      die(63, "Error: %s on chrX / chrY / MT variants is not supported by plink2-hip (filter them away, e.g. --chr 1-22).\n", fl);
    }
  }
  for (uint32_t k = 0; k < S.variant_ct; ++k) {
    if (S.V.alt_ct[S.inc[k]] > 1) {
      die(63, "Error: %s on multiallelic variants is not supported by plink2-hip.\n", fl);
    }
  }
  if (ldp_pgen_has_dosage(S.pg)) {
    die(63, "Error: %s on a file with dosage tracks is not supported by plink2-hip.\n", fl);
  }
  if (S.founder_ct > ldp_matrix_pipe_max_founders()) {
    die(63, "Error: %s with more than %u founders is not supported by plink2-hip (the matrix-pipe limit).\n", fl, ldp_matrix_pipe_max_founders());
  }
}

// The phase-code rows (include/ldprune_hip.h: ldp_r2_phased_stats_block) of the included variants over the founders, from the file's
// hardcall-phase track -- per sample 00 = phased het, phaseinfo 0; 10 = phased het, phaseinfo 1; 01 = anything else -- in a second
// engine on the plan of the first.  nullptr when no included variant has a phased call (a .bed, a .pgen without the track): the
// reference then reads through PgrGetInv1 and there is nothing to refine.  (The reference decides by the file's header flag; a file
// whose only phased calls sit in variants or samples that were filtered away is the one case in which the two differ.)
ldp_engine* build_phase_engine(Session& S, const ldp_params& RP, const std::vector<double>& cms) {
  const Args& A = S.A;
  if (S.storage_mode == 0x01) {
    return nullptr;
  }
  const uint32_t n = S.raw_sample_ct, m = S.variant_ct;
  std::vector<uint32_t> founder_idx;
  for (uint32_t sx = 0; sx < n; ++sx) {
    if (S.is_founder[sx]) {
      founder_idx.push_back(sx);
    }
  }
  const uint64_t rec = (static_cast<uint64_t>(S.founder_ct) + 3) / 4;
  std::vector<uint8_t> rows(static_cast<size_t>(m) * rec, 0);
  std::vector<uint8_t> lo(n), hi(n), pp((n + 7) / 8), pi((n + 7) / 8);
  bool any = false;
  for (uint32_t k = 0; k < m; ++k) {
    if (ldp_pgen_read_alleles_phased(S.pg, S.inc[k], 1, lo.data(), hi.data(), pp.data(), pi.data())) {
      die(6, "Error: %s: %s\n", S.gpath.c_str(), ldp_pgen_last_error(S.pg));
    }
    for (uint8_t b : pp) {
      any = any || (b != 0);
    }
    uint8_t* row = rows.data() + static_cast<size_t>(k) * rec;
    uint32_t f = 0;
    for (uint32_t sx : founder_idx) {
      const bool present = ((pp[sx >> 3] >> (sx & 7)) & 1) && (lo[sx] != hi[sx]);
      const uint32_t code = present ? (((pi[sx >> 3] >> (sx & 7)) & 1) ? 2u : 0u) : 1u;
      row[f >> 2] |= static_cast<uint8_t>(code << (2 * (f & 3)));
      ++f;
    }
  }
  if (!any) {
    return nullptr;
  }
  ldp_engine* ph = nullptr;
  if (ldp_create(&RP, &ph) || ldp_set_variants_vcor_cm(ph, m, S.chr_idx.data(), S.bps.data(), cms.empty() ? nullptr : cms.data(), A.ld_bp_radius, A.ld_cm_radius,
                                                       A.ld_var_ct_radius)) {
    die(16, "Error: engine setup failed%s%s\n", ph ? ": " : ".", ph ? ldp_last_error(ph) : "");
  }
  if (ldp_load_genotypes(ph, 0, m, rows.data(), rec, LDP_MEM_HOST, LDP_GENO_REF)) {
    die(16, "Error: %s\n", ldp_last_error(ph));
  }
  return ph;
}

namespace {
// The same pair with the other allele of its first (which = 0) or second (which = 1) variant counted: the sum becomes 2 n - sum, and the
// haplotypes known to carry both counted alleles become those that carried the OTHER variant's counted allele alone, sum_other - known -
// unknown (the f12 / f21 of ldp_phased_ld.cpp); the double heterozygotes stay what they are.
void count_other_allele(ldp_phased_stats_t* s, int which) {
  uint32_t& mine = which ? s->sum1 : s->sum0;
  const uint32_t other = which ? s->sum0 : s->sum1;
  s->known_dotprod = other - s->known_dotprod - s->unknown_hethet;
  mine = 2 * s->valid_obs - mine;
}
}  // namespace

int write_vcor_table_phased(R2Job& J, ldp_engine* phase) {
  Session& S = J.S;
  const Args& A = S.A;
  const Variants& V = S.V;
  ldp_engine* const e = J.e;
  const std::vector<uint32_t>&inc = S.inc, &chr_idx = S.chr_idx;
  const uint32_t variant_ct = S.variant_ct;
  const char* fl = A.r_unsquared ? "--r-phased" : "--r2-phased";
  std::vector<uint32_t> lo(std::max<uint32_t>(variant_ct, 1));
  uint64_t cand = 0;
  ldp_get_band(e, lo.data(), &cand);
  const std::string tpath = A.out + ".vcor" + (A.r2_zs ? ".zst" : "");
  OutFile tf;
  tf.open(tpath, A.r2_zs);
  const VcorColumns columns(J);
  {
    const std::string hdr = columns.header();
    tf.write(hdr.data(), hdr.size());
  }
  // (--r-phased filters |r| against the root of --ld-window-r2, like its unphased twin: VcorTable :11575-11579)
  const double thresh = A.r_unsquared ? ((A.ld_min_r2 < 0.0) ? -1.0 : sqrt(A.ld_min_r2)) : A.ld_min_r2;
  const std::vector<uint8_t> is_row = vcor_row_variants(A, V, inc, variant_ct, thresh);
  const bool row_subset = !is_row.empty();
  // 'ref-based': the reference counts REF-vs-ALT instead of major-vs-rest -- ALT through PgrGetInv1, REF through PgrGetInv1P (which hands
  // its caller the complement, pgenlib_read.cc:7016-7042).  The engines count the non-major allele (no phase rows) or the major one
  // (phase rows); where that is not the allele wanted the pair's integers are turned over on the host, exactly.
  std::vector<uint8_t> turn;
  if (A.r2_ref_based) {
    std::vector<ldp_variant_rec> recs(variant_ct);
    if (variant_ct && ldp_get_variant_recs(e, 0, variant_ct, recs.data())) {
      die(16, "Error: %s\n", ldp_last_error(e));
    }
    turn.resize(variant_ct);
    for (uint32_t k = 0; k < variant_ct; ++k) {
      // counted now: ALT when (ALT is major) == (phase rows); wanted: ALT without phase rows, REF with them -- they differ where ALT is major
      turn[k] = static_cast<uint8_t>(recs[k].flags & 1u);
    }
  }
  struct Line {
    uint32_t a, b;
    double v, d, dprime;
  };
  std::vector<Line> lines;
  uint64_t capacity = 1ull << 22;
  std::vector<ldp_phased_stats_t> st(capacity);
  std::vector<uint32_t> hf(capacity), hs(capacity);
  std::vector<double> r2, d, dp;
  std::vector<uint8_t> neg;
  uint64_t seen = 0, dropped = 0;
  double ms_hethet = 0.0, ms_tuples = 0.0, ms_em = 0.0;
  uint32_t rows_per = 65536;
  for (uint32_t r0 = 0; r0 < variant_ct;) {
    const uint32_t rows = std::min(rows_per, variant_ct - r0);
    uint64_t found = 0;
    // (a negative threshold keeps every defined pair: the device-side bound is asked for 0, which drops nothing)
    if (ldp_r2_phased_band_hits(e, phase, r0, rows, std::max(thresh, 0.0), A.r_unsquared ? 1 : 0, st.data(), hf.data(), hs.data(), capacity, &found)) {
      die(16, "Error: %s\n", ldp_last_error(e));
    }
    if (found > capacity) {
      if (rows == 1) {
        die(2, "Error: one variant has more partners than the filter buffer holds.\n");
      }
      rows_per = std::max(1u, rows / 2);  // more survivors than the buffer holds: fewer second variants per call
      continue;
    }
    {
      uint64_t s0 = 0, s1 = 0;
      double t0 = 0.0, t1 = 0.0;
      (void)ldp_debug_get_phased_filter(e, &s0, &s1, &t0, &t1);
      seen += s0;
      dropped += s1;
      ms_hethet += t0;
      ms_tuples += t1;
    }
    // the line's A is the lower index, or with --ld-snp the row variant (VcorTableWriteThread :10806-10815); the statistic takes its
    // variants in the line's order (the cubic's coefficients do not round symmetrically)
    for (uint64_t q = 0; q < found; ++q) {
      if (row_subset) {
        if (!is_row[hf[q]] && !is_row[hs[q]]) {
          hf[q] = 0xffffffffu;
          continue;
        }
        if (!is_row[hf[q]]) {
          std::swap(hf[q], hs[q]);
          std::swap(st[q].sum0, st[q].sum1);
        }
      }
      if (A.r2_ref_based) {
        if (turn[hf[q]]) {
          count_other_allele(&st[q], 0);
        }
        if (turn[hs[q]]) {
          count_other_allele(&st[q], 1);
        }
      }
    }
    r2.resize(found);
    d.resize(found);
    dp.resize(found);
    neg.resize(found);
    const auto t_em = std::chrono::steady_clock::now();
    if (found && ldp_phased_ld(st.data(), found, r2.data(), d.data(), dp.data(), neg.data())) {
      die(16, "Error: ldp_phased_ld failed.\n");
    }
    ms_em += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_em).count();
    for (uint64_t q = 0; q < found; ++q) {
      if ((hf[q] == 0xffffffffu) || (r2[q] != r2[q])) {
        continue;  // (an undefined pair is never printed: ComputeR2 hands back -DBL_MAX, plink2_ld.cc:6708-6726)
      }
      double v = r2[q];
      if (A.r_unsquared) {
        v = sqrt(v);
        if (neg[q]) {
          v = -v;
        }
      }
      if ((thresh >= 0.0) && (!(fabs(v) >= thresh))) {  // VcorTableWriteThread :10816-10821
        continue;
      }
      lines.push_back({hf[q], hs[q], v, d[q], dp[q]});
    }
    r0 += rows;
  }
  std::sort(lines.begin(), lines.end(), [](const Line& x, const Line& y) { return (x.a != y.a) ? (x.a < y.a) : (x.b < y.b); });
  std::vector<std::string> chr_name;  // by chromosome order index
  for (uint32_t k = 0; k < variant_ct; ++k) {
    if (chr_idx[k] >= chr_name.size()) {
      chr_name.resize(chr_idx[k] + 1);
      chr_name[chr_idx[k]] = vcor_chrom_name(V.chrom[inc[k]]);
    }
  }
  std::string out;
  out.reserve(1 << 22);
  char num[40];
  for (const Line& ln : lines) {
    columns.put(ln.a, chr_name[chr_idx[ln.a]], &out);
    columns.put(ln.b, chr_name[chr_idx[ln.b]], &out);
    out.append(num, format_g6(ln.v, num) - num);
    if (columns.cols & kVcorColD) {
      out += '\t';
      out.append(num, format_g6(ln.d, num) - num);
    }
    if (columns.cols & (kVcorColDprimeAbs | kVcorColDprime)) {
      out += '\t';
      out.append(num, format_g6((columns.cols & kVcorColDprimeAbs) ? fabs(ln.dprime) : ln.dprime, num) - num);
    }
    out += '\n';
    if (out.size() > (1u << 21)) {
      tf.write(out.data(), out.size());
      out.clear();
    }
  }
  tf.write(out.data(), out.size());
  tf.close();
  logprintf("%s: %llu variant pair%s written to %s .\n", fl, static_cast<unsigned long long>(lines.size()), lines.size() == 1 ? "" : "s", tpath.c_str());
  if (A.timing) {
    fprintf(stderr, "timing: %s double-heterozygote kernel %.3f ms, six-integer launches %.3f ms, bound dropped %llu of %llu pairs, host EM %.3f ms\n", fl, ms_hethet, ms_tuples,
            static_cast<unsigned long long>(dropped), static_cast<unsigned long long>(seen), ms_em);
  }
  if (phase) {
    ldp_destroy(phase);
  }
  ldp_destroy(e);
  ldp_pgen_close(S.pg);
  if (g_log) {
    fclose(g_log);
  }
  return 0;
}

}  // namespace p2h
