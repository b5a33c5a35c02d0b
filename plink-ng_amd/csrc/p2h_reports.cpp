// p2h_reports.cpp -- plink2-hip: the count reports.  --missing (.smiss / .vmiss: WriteMissingnessReports, plink2_misc.cc:4560-4970), --freq
// (.afreq / .acount: WriteAlleleFreqs, :3560-3960) and --geno-counts (.gcount: WriteGenoCounts, :4040-4400) with their default columns.  The
// reference writes them after the sample filters and before --geno / --maf / --mac, over every variant the table filters leave; one writer
// here, fed by whichever pass counted: the host's over the rows (load_inputs) or the records the device's count pass left (run_prune).
#include "p2h_r2_job.h"

namespace p2h {

namespace {

bool missing_pheno_token(const std::string& t) { return (t == "-9") || ieq(t.c_str(), "NA") || ieq(t.c_str(), "nan"); }

// the name of a phenotype the reference would load from the sample file (it then prints a column per phenotype into .smiss); empty: none.  A .fam's sixth
// column counts when it holds a value; a .psam's phenotype column counts as soon as it is there (the reference keeps a named column without values)
std::string loaded_phenotype(const Args& A) {
  const bool psam = !A.psam.empty();
  std::ifstream in(psam ? A.psam : A.fam);
  std::string line;
  std::vector<std::string> names;
  bool header_seen = false;
  while (std::getline(in, line)) {
    if (line.empty()) {
      continue;
    }
    if (psam && (line[0] == '#')) {
      if ((line.rfind("#FID", 0) == 0) || (line.rfind("#IID", 0) == 0)) {
        const std::vector<std::string> h = split_ws(line);
        for (size_t c = 1; c < h.size(); ++c) {
          if ((h[c] != "IID") && (h[c] != "SID") && (h[c] != "PAT") && (h[c] != "MAT") && (h[c] != "SEX")) {
            names.push_back(h[c]);
          }
        }
        header_seen = true;
      }
      continue;
    }
    const std::vector<std::string> t = split_ws(line);
    if ((!psam) || !header_seen) {  // .fam layout: FID IID PAT MAT SEX PHENO
      if ((t.size() > 5) && !missing_pheno_token(t[5])) {
        return "PHENO1";
      }
      continue;
    }
    break;
  }
  return names.empty() ? std::string() : names[0];
}

char* put_u32(uint32_t v, char* out) { return out + sprintf(out, "%u", v); }

struct ProvRef {
  int storage = 1;  // ldp_pgen_provisional_ref: 1 none, 2 all, 3 per variant
  std::vector<uint8_t> bits;
  bool column = false;  // the 'maybeprovref' rule (ProvrefCol, plink2_common.h:1549): the column appears when some listed REF is provisional
  bool of(uint32_t v) const { return (storage == 2) || ((storage == 3) && ((v >> 3) < bits.size()) && ((bits[v >> 3] >> (v & 7)) & 1)); }
};

ProvRef provisional_refs(const Session& S, const std::vector<uint32_t>& listed) {
  ProvRef P;
  P.bits.assign((static_cast<size_t>(S.V.id.size()) + 7) / 8, 0);
  P.storage = ldp_pgen_provisional_ref(S.pg, P.bits.data(), P.bits.size());
  if ((P.storage == 0) && S.V.info_pr_header) {  // the .pgen leaves it to the .pvar's INFO/PR
    P.storage = 3;
    std::copy(S.V.info_pr.begin(), S.V.info_pr.begin() + std::min(S.V.info_pr.size(), P.bits.size()), P.bits.begin());
  }
  P.column = (P.storage == 2);
  for (size_t q = 0; (P.storage == 3) && (!P.column) && (q < listed.size()); ++q) {
    P.column = P.of(listed[q]);
  }
  return P;
}

// chromosome names as the reference prints them, looked up once per run of variants on one chromosome
struct ChromNames {
  const Variants& V;
  const std::string* last = nullptr;
  std::string out;
  explicit ChromNames(const Variants& v) : V(v) {}
  const std::string& of(uint32_t raw) {
    if ((!last) || (*last != V.chrom[raw])) {
      last = &V.chrom[raw];
      out = vcor_chrom_name(*last);
    }
    return out;
  }
};

}  // namespace

void reports_list_variants(Session& S, VariantFilter& filter, std::vector<uint32_t>* listed) {
  const Args& A = S.A;
  const Variants& V = S.V;
  const char* what = A.rep_missing ? "--missing" : (A.rep_freq ? "--freq" : "--geno-counts");
  if (ldp_pgen_has_dosage(S.pg)) {
    // (the reference counts dosages where a record has them -- ALT_FREQS, OBS_CT and the missing-dosage columns' cousins: plink2_data.cc:2421-2443)
    die(63, "Error: %s holds dosage data, which the reports of plink2-hip (%s) do not read.  Use plink2 --make-pgen erase-dosage first.\n", S.gpath.c_str(), what);
  }
  if (A.rep_smiss()) {
    const std::string pheno = loaded_phenotype(A);
    if (!pheno.empty()) {
      die(63, "Error: the sample file carries a phenotype ('%s'), and the phenotype columns of .smiss are not supported by plink2-hip: use --missing variant-only, or plink2.\n", pheno.c_str());
    }
  }
  listed->clear();
  filter.walk(
      [&](const std::string& cur, const ChromFacts& c) {
        if ((!c.out) && (c.cls == 2)) {
          die(6, "Error: Invalid chromosome code '%s'. (Use --allow-extra-chr to force it to be accepted.)\n", cur.c_str());
        }
        if ((!c.out) && (c.cls >= 3)) {
          // (the haploid genotype columns, the male-only observation counts of chrY and the chrX allele weights are not built)
          die(63, "Error: %s with chrX, chrY or MT variants ('%s') is not supported by plink2-hip: filter them out (--autosome, --chr, --not-chr) or use plink2.\n", what, cur.c_str());
        }
      },
      [&](uint32_t v, const ChromFacts&) {
        if (A.rep_gcount && (V.alt_ct[v] > 1)) {
          // (HET_REF_ALT_CTS / TWO_ALT_GENO_CTS list every genotype pair of the alleles: nobody counts those here)
          die(63, "Error: --geno-counts with a multiallelic variant ('%s') is not supported by plink2-hip: --max-alleles 2 leaves them out.\n", V.id[v].c_str());
        }
        listed->push_back(v);
      });
}

void reports_count_alleles_host(const Session& S, uint32_t raw_variant, std::vector<uint8_t>* lo, std::vector<uint8_t>* hi, std::vector<uint32_t>* counts) {
  const uint32_t alts = S.V.alt_ct[raw_variant];
  const uint32_t n = static_cast<uint32_t>(S.is_founder.size());
  lo->resize(n);
  hi->resize(n);
  if (ldp_pgen_read_alleles(S.pg, raw_variant, alts, lo->data(), hi->data())) {
    die(6, "Error: %s: %s\n", S.gpath.c_str(), ldp_pgen_last_error(S.pg));
  }
  counts->assign(alts + 1, 0);
  for (uint32_t s = 0; s < n; ++s) {
    if (S.is_founder[s] && ((*lo)[s] != 255)) {
      if (((*lo)[s] > alts) || ((*hi)[s] > alts)) {
        die(6, "Error: %s: variant '%s' names an allele its .pvar line does not have.\n", S.gpath.c_str(), S.V.id[raw_variant].c_str());
      }
      ++(*counts)[(*lo)[s]];
      ++(*counts)[(*hi)[s]];
    }
  }
}

void write_reports(const Session& S, const ReportCounts& C) {
  const Args& A = S.A;
  const Variants& V = S.V;
  const size_t n = C.variants.size();
  char num[64];
  std::string buf;
  auto flush = [&](OutFile& f, bool force) {
    if (force || (buf.size() > (1u << 20))) {
      f.write(buf.data(), buf.size());
      buf.clear();
    }
  };
  ProvRef P;
  if (A.rep_freq || A.rep_gcount) {
    P = provisional_refs(S, C.variants);
  }
  auto variant_columns = [&](ChromNames& names, uint32_t v) {  // #CHROM ID REF ALT [PROVISIONAL_REF?]
    buf += names.of(v);
    buf += '\t';
    buf += V.id[v];
    buf += '\t';
    buf += V.ref[v];
    buf += '\t';
    buf += V.alt[v];
    if (P.column) {
      buf += P.of(v) ? "\tY" : "\tN";
    }
  };
  if (A.rep_freq) {
    const std::string path = A.out + (A.rep_freq_counts ? ".acount" : ".afreq") + (A.rep_freq_zs ? ".zst" : "");
    OutFile f;
    f.open(path, A.rep_freq_zs);
    buf = "#CHROM\tID\tREF\tALT";
    buf += P.column ? "\tPROVISIONAL_REF?" : "";
    buf += A.rep_freq_counts ? "\tALT_CTS\tOBS_CT\n" : "\tALT_FREQS\tOBS_CT\n";
    ChromNames names(V);
    std::vector<uint32_t> two(2);
    for (size_t q = 0; q < n; ++q) {
      const uint32_t v = C.variants[q];
      variant_columns(names, v);
      const std::vector<uint32_t>* cts = &two;
      const auto multi = C.allele_cts.find(static_cast<uint32_t>(q));
      if (multi != C.allele_cts.end()) {
        cts = &multi->second;
      } else {
        two[0] = 2 * C.f_ref2[q] + C.f_het[q];
        two[1] = 2 * C.f_alt2[q] + C.f_het[q];
      }
      uint64_t tot = 0;
      for (uint32_t c : *cts) {
        tot += c;
      }
      // (WriteAlleleFreqs :3750-3785: count * (1 / total); nothing observed: 0 * inf = nan)
      const double tot_recip = 1.0 / static_cast<double>(tot);
      for (size_t a = 1; a < cts->size(); ++a) {
        buf += (a == 1) ? '\t' : ',';
        char* e = A.rep_freq_counts ? put_u32((*cts)[a], num) : format_g6(static_cast<double>((*cts)[a]) * tot_recip, num);
        buf.append(num, e);
      }
      buf += '\t';
      buf.append(num, static_cast<size_t>(sprintf(num, "%llu", static_cast<unsigned long long>(tot))));
      buf += '\n';
      flush(f, false);
    }
    flush(f, true);
    f.close();
    logprintf("--freq%s: Allele %s (founders only) written to %s .\n", A.rep_freq_counts ? " counts" : "", A.rep_freq_counts ? "counts" : "frequencies", path.c_str());
  }
  if (A.rep_gcount) {
    const std::string path = A.out + ".gcount" + (A.rep_gcount_zs ? ".zst" : "");
    OutFile f;
    f.open(path, A.rep_gcount_zs);
    buf = "#CHROM\tID\tREF\tALT";
    buf += P.column ? "\tPROVISIONAL_REF?" : "";
    buf += "\tHOM_REF_CT\tHET_REF_ALT_CTS\tTWO_ALT_GENO_CTS\tHAP_REF_CT\tHAP_ALT_CTS\tMISSING_CT\n";
    ChromNames names(V);
    const bool same = C.s_ref2.empty();  // (the kept samples are the founders)
    for (size_t q = 0; q < n; ++q) {
      variant_columns(names, C.variants[q]);
      const uint32_t vals[6] = {same ? C.f_ref2[q] : C.s_ref2[q], same ? C.f_het[q] : C.s_het[q], same ? C.f_alt2[q] : C.s_alt2[q], 0, 0, C.missing[q]};
      for (uint32_t x : vals) {
        buf += '\t';
        buf.append(num, put_u32(x, num));
      }
      buf += '\n';
      flush(f, false);
    }
    flush(f, true);
    f.close();
    logprintf("--geno-counts: Genotype counts written to %s .\n", path.c_str());
  }
  if (A.rep_smiss()) {
    const std::string path = A.out + ".smiss" + (A.rep_missing_zs ? ".zst" : "");
    OutFile f;
    f.open(path, A.rep_missing_zs);
    buf = S.fid_present ? "#FID\tIID" : "#IID";
    buf += S.sample_sids.empty() ? "" : "\tSID";
    buf += "\tMISSING_CT\tOBS_CT\tF_MISS\n";
    const uint32_t variant_ct = static_cast<uint32_t>(n);
    const double variant_ct_recip = 1.0 / static_cast<double>(variant_ct);  // (:4702)
    char obs[16];
    const size_t obs_len = static_cast<size_t>(put_u32(variant_ct, obs) - obs);
    for (size_t sx = 0; sx < S.is_founder.size(); ++sx) {
      if ((!S.sample_kept.empty()) && !S.sample_kept[sx]) {
        continue;
      }
      buf += S.sample_keys[sx].c_str() + (S.fid_present ? 0 : 2);  // (no FID column: every key starts with "0<tab>")
      if (!S.sample_sids.empty()) {
        buf += '\t';
        buf += S.sample_sids[sx];
      }
      buf += '\t';
      buf.append(num, put_u32(C.sample_missing[sx], num));
      buf += '\t';
      buf.append(obs, obs_len);
      buf += '\t';
      buf.append(num, format_g6(static_cast<double>(C.sample_missing[sx]) * variant_ct_recip, num));
      buf += '\n';
      flush(f, false);
    }
    flush(f, true);
    f.close();
    logprintf("--missing: Sample missing data report written to %s .\n", path.c_str());
  }
  if (A.rep_vmiss()) {
    const std::string path = A.out + ".vmiss" + (A.rep_missing_zs ? ".zst" : "");
    OutFile f;
    f.open(path, A.rep_missing_zs);
    buf = "#CHROM\tID\tMISSING_CT\tOBS_CT\tF_MISS\n";
    const double nobs_recip = 1.0 / static_cast<double>(C.kept_sample_ct);  // (:4874)
    char obs[16];
    const size_t obs_len = static_cast<size_t>(put_u32(C.kept_sample_ct, obs) - obs);
    ChromNames names(V);
    for (size_t q = 0; q < n; ++q) {
      const uint32_t v = C.variants[q];
      buf += names.of(v);
      buf += '\t';
      buf += V.id[v];
      buf += '\t';
      buf.append(num, put_u32(C.missing[q], num));
      buf += '\t';
      buf.append(obs, obs_len);
      buf += '\t';
      buf.append(num, format_g6(static_cast<double>(C.missing[q]) * nobs_recip, num));
      buf += '\n';
      flush(f, false);
    }
    flush(f, true);
    f.close();
    logprintf("--missing: Variant missing data report written to %s .\n", path.c_str());
  }
}

// --hardy (HardyReport, plink2_misc.cc:5397-5687) with its default columns: one line per listed variant, A1 = REF and AX = ALT, the founders'
// three genotype counts, observed and expected het frequency as the reference forms them (:5641-5655: a variant nobody has a call at
// prints 0 * (1 / 0) = nan and, its A1 homozygotes being all of its calls, 0), and the p-value printed from its logarithm, so that values
// far below DBL_MIN print as the reference's do.  No file when nothing is listed.
void write_hardy(const Session& S, const HardyCounts& H) {
  const Args& A = S.A;
  const Variants& V = S.V;
  if (H.haploid_skipped) {
    logprintf("--hardy: Skipping %u haploid variant%s.\n", H.haploid_skipped, (H.haploid_skipped == 1) ? "" : "s");
  }
  const size_t n = H.variants.size();
  if (!n) {
    return;
  }
  const std::string path = A.out + ".hardy" + (A.hardy_zs ? ".zst" : "");
  OutFile f;
  f.open(path, A.hardy_zs);
  char num[64];
  std::string buf = "#CHROM\tID\tA1\tAX\tHOM_A1_CT\tHET_A1_CT\tTWO_AX_CT\tO(HET_A1)\tE(HET_A1)\t";
  buf += A.hardy_midp ? "MIDP\n" : "P\n";
  ChromNames names(V);
  for (size_t q = 0; q < n; ++q) {
    const uint32_t v = H.variants[q];
    buf += names.of(v);
    buf += '\t';
    buf += V.id[v];
    buf += '\t';
    buf += V.ref[v];
    buf += '\t';
    buf += V.alt[v];
    const uint32_t cts[3] = {H.hom1[q], H.het[q], H.hom2[q]};
    for (uint32_t x : cts) {
      buf += '\t';
      buf.append(num, put_u32(x, num));
    }
    const uint32_t nonmissing = cts[0] + cts[1] + cts[2];
    const double recip = 1.0 / static_cast<double>(nonmissing);
    buf += '\t';
    buf.append(num, format_g6(static_cast<double>(cts[1]) * recip, num));
    buf += '\t';
    if (cts[0] == nonmissing) {
      buf += '0';
    } else {
      const double dbl_maj_freq = static_cast<double>(cts[0] * 2 + cts[1]) * recip;
      buf.append(num, format_g6(dbl_maj_freq * (1.0 - dbl_maj_freq * 0.5), num));
    }
    buf += '\t';
    buf.append(num, format_ln_g6(H.ln_p[q], num));
    buf += '\n';
    if (buf.size() > (1u << 20)) {
      f.write(buf.data(), buf.size());
      buf.clear();
    }
  }
  f.write(buf.data(), buf.size());
  f.close();
  logprintf_ww("--hardy%s%s: Autosomal Hardy-Weinberg report (founders only) written to %s .\n", A.hardy_zs ? " zs" : "", A.hardy_midp ? " midp" : "", path.c_str());
}

}  // namespace p2h
