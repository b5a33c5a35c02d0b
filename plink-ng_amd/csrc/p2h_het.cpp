// p2h_het.cpp -- plink2-hip: --het, the per-sample inbreeding coefficient (HetReport / HetCalcMain / HetThread, plink2_misc.cc:9774-10501) with
// its default columns.  The reference runs it after every sample and variant filter, right behind the prune, over the autosomal variants the
// filters leave: per variant an expected heterozygosity ehet_v from the founders' allele counts, per sample the variants it has a call at
// (nobs), the ones where it is heterozygous (ohet) and the sum of ehet_v over the former (ehet); F = 1 - ohet / ehet.
//
// The reference sums ehet in doubles, per thread and in file order, so its last bits depend on its thread count.  Here the sum is made of
// integers (HetPlan): exact, the same in any order, and so the same from the device's pass over the resident image (run_prune:
// ldp_sample_het_counts, which sums the q_v of a sample's missing calls modulo 2^64) and from the host's pass over the rows (het_host_pass,
// p2h_inputs.cpp).  Every q_v is within 1/2 of ehet_v * 2^k, so a sample's ehet is within m * 2^-(k+1) of the exact sum: m * 2^-53 while
// m < 1024 (k = 52; a double sum of m terms below 1 errs by up to m * (m / 2) * 2^-53), and never more than 2^-30 relative to m for any m
// below 2^32 (k = 62 - bit_length(m) >= 30).
#include "p2h_cli.h"

namespace p2h {

void logprintf_ww(const char* fmt, ...) {
  char buf[4096];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  // WordWrap (plink2_string.cc:212): a line holds 79 characters; a space that a token would cross the limit behind becomes the line's end
  for (char* line = buf; *line;) {
    char* eol = strchr(line, '\n');
    char* end = eol ? eol : line + strlen(line);
    char* start = line;
    char* last_space = nullptr;
    for (char* p = line; p <= end; ++p) {
      if ((p == end) || (*p == ' ')) {
        const size_t visible = static_cast<size_t>(p - start);
        if ((visible > 79) && last_space) {
          *last_space = '\n';
          start = last_space + 1;
        }
        last_space = (p == end) ? nullptr : p;
      }
    }
    line = eol ? eol + 1 : end;
  }
  logprintf("%s", buf);
}

bool het_expected(const uint32_t* cts, uint32_t allele_ct, bool small_sample, double* ehet) {
  constexpr double k2m35 = 1.0 / 34359738368.0;
  uint64_t tot = 0;
  for (uint32_t a = 0; a < allele_ct; ++a) {
    tot += cts[a];
  }
  if (!small_sample) {
    // ComputeAlleleFreqs (plink2_filter.cc:2113-2150): count * (1 / total), nothing observed: 1 / alleles each; HetThread :9875-9881, :9994-10010
    const double recip = tot ? (1.0 / static_cast<double>(tot)) : 0.0;
    const double none = 1.0 / static_cast<double>(allele_ct);
    if (allele_ct == 2) {
      const double ref_freq = tot ? (static_cast<double>(cts[0]) * recip) : none;
      *ehet = 2 * ref_freq * (1 - ref_freq);
    } else {
      double freq_sum = 0.0, freq_ssq = 0.0;
      for (uint32_t a = 0; a + 1 < allele_ct; ++a) {
        const double f = tot ? (static_cast<double>(cts[a]) * recip) : none;
        freq_sum += f;
        freq_ssq += f * f;
      }
      const double last = 1.0 - freq_sum;
      *ehet = 1.0 - freq_ssq - last * last;
    }
    return !(*ehet < k2m35);
  }
  if (allele_ct == 2) {  // :9920-9927
    const uint32_t numer1 = cts[0], numer2 = cts[1];
    if ((!numer1) || (!numer2)) {
      return false;
    }
    const uint32_t denom = numer1 + numer2;
    *ehet = 2 * static_cast<double>(numer1) * static_cast<double>(numer2) / (static_cast<double>(denom) * static_cast<double>(denom - 1));
    return true;
  }
  if (!tot) {  // :10023-10027 (one allele alone is not skipped there: its ehet is 0)
    return false;
  }
  uint64_t ssq = 0;
  for (uint32_t a = 0; a < allele_ct; ++a) {
    ssq += static_cast<uint64_t>(cts[a]) * cts[a];
  }
  const double denom_d = static_cast<double>(static_cast<uint32_t>(tot));
  *ehet = (1.0 - (static_cast<double>(ssq) / (denom_d * denom_d))) * (denom_d / static_cast<double>(static_cast<uint32_t>(tot) - 1));
  return true;
}

void HetPlan::build(const std::vector<double>& ehet, const std::vector<uint8_t>& ok) {
  const size_t n = ehet.size();
  kept = skipped = 0;
  for (size_t v = 0; v < n; ++v) {
    (ok[v] ? kept : skipped) += 1;
  }
  int bits = 0;
  while ((static_cast<uint64_t>(kept) >> bits) != 0) {
    ++bits;
  }
  k = std::min(52, 62 - bits);
  weight.assign(n, 0);
  include.assign(n, 0);
  total = 0;
  for (size_t v = 0; v < n; ++v) {
    if (ok[v]) {
      // (ehet_v <= 1: at most 2^k each, below 2^62 together; exact for k = 52 only where ehet_v has no bit below 2^-52 -- the rounding is the bound above)
      const double scaled = std::ldexp(ehet[v], k);
      const uint64_t q = (scaled > 0.0) ? static_cast<uint64_t>(std::llrint(scaled)) : 0;
      weight[v] = q;
      include[v] = 1;
      total += q;
    }
  }
}

void het_preamble(const Session& S, uint32_t autosomal, uint32_t non_autosomal) {
  const Args& A = S.A;
  if (A.het_small_sample && !S.founder_ct) {  // :10389-10392
    die(7, "Error: '--het small-sample' requires founders.  (--make-founders may come in\nhandy here.\n)");
  }
  if (non_autosomal) {  // ConditionalAllocateNonAutosomalVariants, plink2_common.cc:3375-3387
    logprintf("Excluding %u variant%s on non-autosomes from --het.\n", non_autosomal, (non_autosomal == 1) ? "" : "s");
  }
  if (!autosomal) {
    if (non_autosomal) {
      logprintf("Error: No variants remaining for --het.\n");
    }
    die(7, "Error: --het requires at least one polymorphic autosomal variant.\n");
  }
}

void het_write(const Session& S, const HetPlan& plan, const HetSums& sums) {
  const Args& A = S.A;
  logprintf("--het: done.\n");
  if (plan.skipped) {  // HetCalcMain :10353-10355
    logprintf_ww("Warning: %u variant%s skipped because %s monomorphic.%s\n", plan.skipped, (plan.skipped == 1) ? "" : "s", (plan.skipped == 1) ? "it was" : "they were",
                 A.het_small_sample ? "" : " You may want to use --read-freq to provide more accurate allele frequency estimates.");
  }
  const std::string path = A.out + ".het" + (A.het_zs ? ".zst" : "");
  OutFile f;
  f.open(path, A.het_zs);
  std::string buf = S.fid_present ? "#FID\tIID" : "#IID";
  buf += S.sample_sids.empty() ? "" : "\tSID";
  buf += "\tO(HOM)\tE(HOM)\tOBS_CT\tF\n";
  char num[64];
  for (size_t sx = 0; sx < S.is_founder.size(); ++sx) {
    if ((!S.sample_kept.empty()) && !S.sample_kept[sx]) {
      continue;
    }
    buf += S.sample_keys[sx].c_str() + (S.fid_present ? 0 : 2);  // (no FID column: every key starts with "0<tab>")
    if (!S.sample_sids.empty()) {
      buf += '\t';
      buf += S.sample_sids[sx];
    }
    // HetReport :10456-10476
    const uint32_t ohet = sums.het_ct[sx];
    const uint32_t nobs = plan.kept - sums.missing_ct[sx];
    const double ehet = std::ldexp(static_cast<double>(static_cast<int64_t>(plan.total - sums.missing_weight[sx])), -plan.k);
    buf += '\t';
    buf.append(num, static_cast<size_t>(sprintf(num, "%u", nobs - ohet)));
    buf += '\t';
    buf.append(num, format_g6(static_cast<double>(nobs) - ehet, num));
    buf += '\t';
    buf.append(num, static_cast<size_t>(sprintf(num, "%u", nobs)));
    buf += '\t';
    buf.append(num, format_g6(1.0 - static_cast<double>(ohet) / ehet, num));
    buf += '\n';
    if (buf.size() > (1u << 20)) {
      f.write(buf.data(), buf.size());
      buf.clear();
    }
  }
  f.write(buf.data(), buf.size());
  f.close();
  logprintf_ww("--het: Results written to %s .\n", path.c_str());
}

}  // namespace p2h
