// p2h_cli.h -- what the translation units of `plink2-hip` share (p2h_*.cpp, plink2_hip_cli.cpp): the parsed command line, the variant
// and sample tables, the session, the output stream and the helpers one unit calls in another.  Not a public interface.
#ifndef P2H_CLI_H
#define P2H_CLI_H
#include <dlfcn.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cfloat>
#include <fstream>
#include <functional>
#include <sstream>
#include <map>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/ldprune_hip.h"
#include "../../include/ldprune_hip_debug.h"  // (only for the --debug-* test hooks)

namespace p2h {

constexpr double kSmallEpsilon = 0.00000000000005684341886080801486968994140625;  // 2^-44
extern FILE* g_log;
extern bool g_silent;       // --silent
extern bool g_log_mute;     // logprintf() prints nothing (die() still does)
extern bool g_r_unsquared;  // --r-unphased

double now_s();
void logprintf(const char* fmt, ...);
[[noreturn]] void die(int code, const char* fmt, ...);
bool scan_double_plink(const char* s, double* out, const char** endp);
uint32_t banker_round(double v);  // v >= 0, < 2^31
char* put_digits_trimmed(uint32_t u, int digits, int keep, char* out);
char* format_g6(double x, char* out);
char* format_ln_g6(double ln_val, char* out);  // exp(ln_val) as the reference prints p-values (p2h_clump.cpp)

// Output file, optionally Zstandard-compressed ('zs': <name>.zst, as the reference's compress stream writes it;
// plink2_compress_stream.cc).  libzstd.so.1 is bound by hand (no zstd headers in the image); the default compression
// level (3) is used, so the bytes may differ from the reference's file while the decompressed text is identical.
class OutFile {
 public:
  void open(const std::string& path, bool zs) {
    path_ = path;
    f_ = fopen(path.c_str(), "wb");
    if (!f_) {
      die(3, "Error: Failed to open %s for writing.\n", path.c_str());
    }
    if (!zs) {
      return;
    }
    void* lib = dlopen("libzstd.so.1", RTLD_NOW);
    if (!lib) {
      die(63, "Error: 'zs' output needs libzstd.so.1, which could not be loaded.\n");
    }
    create_ = reinterpret_cast<void* (*)()>(dlsym(lib, "ZSTD_createCCtx"));
    destroy_ = reinterpret_cast<size_t (*)(void*)>(dlsym(lib, "ZSTD_freeCCtx"));
    step_ = reinterpret_cast<size_t (*)(void*, Buf*, CBuf*, int)>(dlsym(lib, "ZSTD_compressStream2"));
    is_error_ = reinterpret_cast<unsigned (*)(size_t)>(dlsym(lib, "ZSTD_isError"));
    if (!create_ || !destroy_ || !step_ || !is_error_) {
      die(63, "Error: libzstd.so.1 lacks the streaming compression API.\n");
    }
    ctx_ = create_();
    if (!ctx_) {
      die(2, "Error: Out of memory.\n");
    }
    obuf_.resize(1 << 20);
  }
  void write(const void* p, size_t n) {
    if (!ctx_) {
      if (n && (fwrite(p, 1, n, f_) != n)) {
        die(5, "Error: File write failure: %s.\n", path_.c_str());
      }
      return;
    }
    pump(p, n, 0);
  }
  void close() {
    if (ctx_) {
      pump(nullptr, 0, 2);  // ZSTD_e_end
      destroy_(ctx_);
      ctx_ = nullptr;
    }
    if (fclose(f_)) {
      die(5, "Error: File write failure: %s.\n", path_.c_str());
    }
    f_ = nullptr;
  }

 private:
  struct Buf {
    void* dst;
    size_t size, pos;
  };
  struct CBuf {
    const void* src;
    size_t size, pos;
  };
  void pump(const void* p, size_t n, int end_op) {
    CBuf in{p, n, 0};
    while (true) {
      Buf out{obuf_.data(), obuf_.size(), 0};
      const size_t left = step_(ctx_, &out, &in, end_op);
      if (is_error_(left)) {
        die(5, "Error: zstd compression failure: %s.\n", path_.c_str());
      }
      if (out.pos && (fwrite(obuf_.data(), 1, out.pos, f_) != out.pos)) {
        die(5, "Error: File write failure: %s.\n", path_.c_str());
      }
      if (end_op ? (left == 0) : (in.pos == in.size)) {
        break;
      }
    }
  }
  std::string path_;
  FILE* f_ = nullptr;
  void* ctx_ = nullptr;
  void* (*create_)() = nullptr;
  size_t (*destroy_)(void*) = nullptr;
  size_t (*step_)(void*, Buf*, CBuf*, int) = nullptr;
  unsigned (*is_error_)(size_t) = nullptr;
  std::vector<uint8_t> obuf_;
};

struct Args {
  std::string bed, bim, fam, pgen, pgi, pvar, psam, out = "plink2";
  bool have_prune = false;
  bool pairphase = false;  // --indep-pairphase instead of --indep-pairwise
  uint32_t window = 0, step = 1;
  bool window_is_bp = false;
  double r2 = 0.0;
  int order = 2;
  bool bad_ld = false;
  bool allow_extra_chr = false;
  std::string preferred;
  int gpus = 1;
  bool have_r2 = false;
  uint32_t parallel_idx = 0, parallel_tot = 1;  // --parallel k n (0-based index inside, plink2.cc:10109-10117)
  int r2_shape = -1;      // 0 square, 1 square0, 2 triangle
  int r2_float = -1;      // 1 bin4, 0 bin
  bool yes_really = false;
  bool r2_table = false;   // --r2-unphased without a matrix shape: windowed .vcor table
  bool r2_ref_based = false;
  bool r2_allow_ambiguous = false;
  bool r_unsquared = false;        // --r-unphased: r = +-sqrt(r^2) with the sign of the covariance
  bool r2_phased = false;          // --r2-phased / --r-phased: haplotype-frequency r^2, D, D' (windowed table only; p2h_r2_phased.cpp)
  uint32_t r2_cols = 0;            // kVcorCol* (set after the modifiers are read: plink2.cc:11158-11207)
  std::string r2_cols_desc;        // the text behind cols=
  bool r2_cols_given = false;
  bool r2_zs = false;      // 'zs': Zstandard-compressed table / text matrix
  bool r2_inter = false;   // 'inter-chr': the table over ALL pairs, chromosome 0 included (plink2_ld.cc:11082-11116)
  bool r2_text = false;    // matrix shape without bin/bin4: text matrix
  uint32_t ld_var_ct_radius = 0x7fffffff;  // --ld-window N: N - 1
  uint32_t ld_bp_radius = 0xffffffffu;     // --ld-window-kb; UINT32_MAX = not given (table default 1000 kb)
  double ld_cm_radius = -1.0;              // --ld-window-cm; -1 = not given
  double ld_min_r2 = 2.0;                  // --ld-window-r2 (after the reference's epsilon); 2.0 = not given
  // variant / sample filters applied before the command (the reference's variant_include / sample_include):
  // --chr / --not-chr (codes and code ranges, or names), --autosome, --extract / --exclude (variant ID lists),
  // --keep / --remove (sample ID lists: "FID IID", "IID", or a #FID / #IID header line)
  std::vector<std::string> chr_keep, chr_drop;
  bool autosome = false;
  // --maf / --max-maf (nonmajor-allele frequency over the founders) and --geno (missing-call rate over the samples), as the
  // reference enforces them (EnforceFreqConstraints plink2_filter.cc:3791, EnforceGenoThresh :3498); 0 / 1 / 1 = not given
  double min_maf = 0.0, max_maf = 1.0, geno = 1.0;
  double mind = 1.0;  // --mind (missing-call rate of a sample over the variants the table filters leave; MindFilter plink2_filter.cc:3329); 1 = not given / no-op
  uint64_t min_allele_ddosage = 0, max_allele_ddosage = ~0ull;  // --mac / --max-mac in 32768ths of an allele copy (plink2.cc:8785-8867)
  bool ac_founders = false;
  uint32_t max_alleles = 0xffffffffu;  // --max-alleles N (applied while the variant table loads, LoadPvar)
  bool snps_only = false, snps_only_acgt = false;  // --snps-only ['just-acgt'] (another load-time filter)
  std::vector<std::string> extract_files, exclude_files, keep_files, remove_files;
  // --ld-snp / --ld-snps / --ld-snp-list (plink2.cc:7966-8003): the table's row variants.  ld_snps: (first, second) ID pairs,
  // second empty for a single ID, otherwise the range first..second in file order
  std::vector<std::pair<std::string, std::string>> ld_snps;
  std::string ld_snp_list;
  // --clump (InitClump, plink2_ld.cc:62-78; parsing plink2.cc:4960-5120)
  bool have_clump = false;
  std::vector<std::string> clump_files;  // one or more reports (plink2.cc:4861-4958: comma- or space-separated)
  bool clump_unphased = false;
  bool clump_allow_overlap = false;
  bool clump_no_test = false;
  std::vector<std::string> clump_id_field, clump_p_field, clump_test_field, clump_test;
  bool make_founders = false, make_founders_require2 = false, make_founders_first = false;  // --make-founders ['require-2-missing'] ['first']
  bool clump_zs = false;
  bool clump_force_a1 = false, clump_no_a1 = false;  // --clump-force-a1; --clump-a1-field without names
  std::vector<std::string> clump_a1_field;
  std::string clump_range;                 // --clump-range / --clump-range0 <file>: regions to report overlaps with
  bool clump_range0 = false;
  uint32_t clump_range_border = 0;         // --clump-range-border <kb>, in bp
  bool clump_range_border_given = false;
  bool clump_in_log10 = false, clump_out_log10 = false;  // --clump-log10 ['input-only' | 'output-only']
  bool clump_log10_p1 = false, clump_log10_p2 = false, clump_plain_p1 = false, clump_plain_p2 = false;
  uint32_t clump_cols = 0;                 // kClumpCol* (plink2_ld.h:51-67), set after the modifiers are read
  std::string clump_cols_desc;
  bool clump_cols_given = false;
  std::vector<double> clump_ln_bins;       // --clump-bins: ln of the boundaries, each times (1 + 2^-44); empty: the default four
  double clump_ln_p1 = 2.3025850929940457 * -4.0 * (1.0 - kSmallEpsilon);
  double clump_ln_p2 = 2.3025850929940457 * -2.0 * (1.0 - kSmallEpsilon);
  double clump_r2_raw = 0.5;
  double clump_r2 = 0.5 * (1.0 + kSmallEpsilon);
  uint32_t clump_bp_radius = 249999;
  // the count reports (p2h_reports.cpp): --missing ['zs'] ['sample-only' | 'variant-only'], --freq ['zs'] ['counts'], --geno-counts ['zs']
  bool rep_missing = false, rep_missing_zs = false, rep_sample_only = false, rep_variant_only = false;
  bool rep_freq = false, rep_freq_zs = false, rep_freq_counts = false;
  bool rep_gcount = false, rep_gcount_zs = false;
  bool any_report() const { return rep_missing || rep_freq || rep_gcount; }
  bool rep_smiss() const { return rep_missing && !rep_variant_only; }
  bool rep_vmiss() const { return rep_missing && !rep_sample_only; }
  // --het ['zs'] ['small-sample'] (p2h_het.cpp): after every filter, over the variants they leave -- a command of its own or beside any other
  bool het = false, het_zs = false, het_small_sample = false;
  // --hwe <p> [<k>] ['midp'] ['keep-fewhet'] (a count filter between --geno and --maf / --mac: CountFilters) and its report --hardy ['zs'] ['midp']
  // (p2h_reports.cpp: write_hardy), over what --geno leaves; ln of the threshold as the reference scans it, sample-size term -1 = not given
  bool hwe = false, hwe_midp = false, hwe_keep_fewhet = false;
  double hwe_ln_thresh = 0.0, hwe_sample_size_term = -1.0;
  bool hardy = false, hardy_zs = false, hardy_midp = false;
  // --make-king-table ['zs'] ['counts'] ['cols='...] and --king-table-filter <x> (p2h_king.cpp): the KING-robust table over every pair of kept
  // samples, after every filter -- a command of its own or beside any other
  bool king = false, king_zs = false, king_counts = false, king_cols_given = false, king_filter_given = false;
  uint32_t king_cols = 0;                // kKingCol*
  double king_filter = -DBL_MAX;         // lines with kinship < this are left out
  bool bad_freqs = false;  // --bad-freqs: --het may estimate allele frequencies from fewer than 50 founders (plink2.cc:2076)
  bool timing = false;    // --timing: print per-phase wall times
  bool dry_run = false;  // parse + plan only, print the parameters exactly (%a) and exit: used by the CPU tests
};

std::vector<std::string> split_ws(const std::string& line);
bool ieq(const char* a, const char* b);
const char* scan_ln(const char* s, double* ln_out);  // (--clump section below)

// ---- --r2-unphased cols= (plink2_ld.h:87-101, ParseColDescriptor plink2_cmdline.cc:4375) ----
enum : uint32_t {
  kVcorColChrom = 1u << 0, kVcorColPos = 1u << 1, kVcorColId = 1u << 2, kVcorColRef = 1u << 3, kVcorColAlt1 = 1u << 4, kVcorColAlt = 1u << 5,
  kVcorColMaybeprovref = 1u << 6, kVcorColProvref = 1u << 7, kVcorColMaj = 1u << 8, kVcorColNonmaj = 1u << 9, kVcorColFreq = 1u << 10,
  kVcorColD = 1u << 11, kVcorColDprime = 1u << 12, kVcorColDprimeAbs = 1u << 13,
  kVcorColDefault = kVcorColChrom | kVcorColPos | kVcorColId | kVcorColMaybeprovref
};

enum : uint32_t {
  kClumpColChrom = 1u << 0, kClumpColPos = 1u << 1, kClumpColRef = 1u << 2, kClumpColAlt1 = 1u << 3, kClumpColAlt = 1u << 4,
  kClumpColMaybeprovref = 1u << 5, kClumpColProvref = 1u << 6, kClumpColMaybeA1 = 1u << 7, kClumpColA1 = 1u << 8, kClumpColMaybeF = 1u << 9,
  kClumpColF = 1u << 10, kClumpColTotal = 1u << 11, kClumpColMaybeBounds = 1u << 12, kClumpColBounds = 1u << 13, kClumpColBins = 1u << 14,
  kClumpColSp2 = 1u << 15,
  kClumpColDefault = kClumpColChrom | kClumpColPos | kClumpColMaybeprovref | kClumpColMaybeA1 | kClumpColMaybeF | kClumpColTotal | kClumpColMaybeBounds |
                     kClumpColBins | kClumpColSp2
};

// --make-king-table cols= (plink2_matrix_calc.h: kfKingCol*)
enum : uint32_t {
  kKingColMaybefid = 1u << 0, kKingColFid = 1u << 1, kKingColId = 1u << 2, kKingColMaybesid = 1u << 3, kKingColSid = 1u << 4, kKingColNsnp = 1u << 5,
  kKingColHethet = 1u << 6, kKingColIbs0 = 1u << 7, kKingColIbs1 = 1u << 8, kKingColIbs = 1u << 9, kKingColKinship = 1u << 10,
  kKingColDefault = kKingColMaybefid | kKingColId | kKingColMaybesid | kKingColNsnp | kKingColHethet | kKingColIbs0 | kKingColKinship
};

// test / measurement hooks of the front-end (hidden --debug-* flags; the library itself reads no environment, csrc/ldp_env.h)
struct DebugHooks {
  bool alias_devices = false, x_host = false, host_decode = false, load_map = false, no_bind = false, serial_feed = false;
  bool host_filter = false;  // --debug-host-filter: --geno / --maf / --mac always from the host's own pass over the rows
  uint32_t x_rows = 0, decode_threads = 0;
};
extern DebugHooks g_dbg;

Args parse_args(int argc, char** argv);
// (fid_present / sids: how the reference writes sample ID lists -- WriteSampleIds, plink2_common.cc:4219: an FID column when the file has one,
// a .fam always; an SID column when the .psam has one, else *sids stays empty)
void load_samples(const Args& A, std::vector<uint8_t>* is_founder, std::vector<uint8_t>* sex, std::vector<std::string>* fid_iid = nullptr,
                  std::vector<std::pair<std::string, std::string>>* parents = nullptr, bool* fid_present = nullptr, std::vector<std::string>* sids = nullptr);

struct Variants {
  std::vector<std::string> chrom, id;
  std::vector<uint32_t> bp;
  std::vector<uint8_t> alt_ct;  // number of ALT alleles (1 for biallelic / .bim), capped at 255
  std::vector<uint8_t> alt_missing;  // --max-alleles: the single ALT is a missing code ('.' or '0'), which counts as ONE allele (plink2_pvar.cc:1940-1948); empty unless the filter is on
  std::vector<uint8_t> not_snp; // --snps-only: an allele longer than one character (or, with 'just-acgt', outside ACGT / missing)
  std::vector<std::string> ref, alt;  // allele text (ALT comma-separated as in the file); only kept for --r2-unphased allele columns
  bool info_pr_header = false;        // the .pvar declares INFO/PR as a flag (provisional REF alleles are marked per variant there)
  std::vector<uint8_t> info_pr;       // bit v: variant v's INFO carries PR (PrInInfo, plink2_pvar.cc:561); kept when a REF column is printed
  std::vector<double> cm;             // centimorgan positions; only kept for --ld-window-cm (empty when the file has no CM column)
  bool cm_unsorted = false;           // some chromosome's CM values decrease (LoadPvar, plink2_pvar.cc:2121-2134)
  bool cm_any_nonzero = false;
};

inline uint32_t allele_ct_for_filter(const Variants& V, size_t v) {
  return ((v < V.alt_missing.size()) && V.alt_missing[v]) ? 1u : (static_cast<uint32_t>(V.alt_ct[v]) + 1);
}

std::string slurp(const std::string& path);
// This thread (and every thread it starts from here on) onto the CPUs of the NUMA node the device is attached to; a no-op where the host does not say
// or the node's CPUs are not ours to use.  Returns the node, or -1.
struct AffinityMask {
  bool valid = false;
  unsigned long bits[16] = {0};  // a cpu_set_t (1,024 CPUs)
};
int bind_near_device(int device, AffinityMask* saved = nullptr);
void restore_affinity(const AffinityMask& saved);
void load_variants(const Args& A, Variants* V);
int chrom_class(const std::string& name_in, bool allow_extra, bool* is_zero);
void multiallelic_inverse_row(ldp_pgen* pg, uint32_t raw_variant, uint32_t alt_ct, const std::vector<uint32_t>& founder_idx,
                              std::vector<uint8_t>* lo, std::vector<uint8_t>* hi, uint8_t* out_row, uint64_t out_rec, double* maj_freq,
                              uint8_t* phase = nullptr, uint64_t phase_bytes = 0, bool* unphased = nullptr, uint32_t* maj_idx = nullptr);

// ---- chrX / chrY / MT ---------------------------------------------------------------------------------------
// The reference feeds IndepPairwiseThread differently shaped genotype vectors on these chromosomes
// (plink2_ld.cc:1356-1388): MT/haploid = founders with hets set to missing; chrY = non-female founders, hets to
// missing; chrX = male founders (hets to missing) followed by non-male founders, whose statistics count twice
// (:890-901, :1066-1082).  All of the prune's statistics are sums over samples, so "count twice" is reproduced
// exactly by emitting the non-male block twice; the engine then runs unchanged on founder_ct' samples.
// Allele frequencies follow LoadAlleleAndGenoCountsThread (plink2_data.cc:2421-2700): diploid-style counts over the
// relevant founders (hets count half/half) for MT and chrY, and for chrX non-males weigh twice as much as males
// with a male het counting half (alt = 4*G2 + 2*G1 - 2*M2 - M1 over all / male founders, :2641).
struct SexPlan {
  std::vector<uint32_t> part1;  // samples whose hets become missing
  std::vector<uint32_t> part2;  // chrX non-males (emitted twice); empty otherwise
  bool x_freq = false;
  uint32_t out_ct() const { return static_cast<uint32_t>(part1.size() + 2 * part2.size()); }
};

inline uint32_t code_at(const uint8_t* row, uint32_t s) { return (row[s >> 2] >> (2 * (s & 3))) & 3; }
void build_sex_row(const SexPlan& sp, const uint8_t* raw_row, uint8_t* out_row, uint64_t out_rec, double* maj_freq, const uint8_t* phase = nullptr);
void multiallelic_sex_row(ldp_pgen* pg, uint32_t raw_variant, uint32_t alt_ct, const SexPlan& sp, std::vector<uint8_t>* lo, std::vector<uint8_t>* hi, uint8_t* out_row,
                          uint64_t out_rec, double* maj_freq);
uint32_t sex_major_allele(ldp_pgen* pg, uint32_t raw_variant, uint32_t alt_ct, const SexPlan& sp, std::vector<uint8_t>* lo, std::vector<uint8_t>* hi, double* maj_freq);
void multiallelic_sex_row_phased(ldp_pgen* pg, uint32_t raw_variant, uint32_t alt_ct, const SexPlan& sp, std::vector<uint8_t>* lo, std::vector<uint8_t>* hi, uint8_t* phase,
                                 uint64_t phase_bytes, uint8_t* out_row, uint64_t out_rec, double* maj_freq, bool* unphased);
void fetch_raw_row(ldp_pgen* pg, int storage_mode, uint32_t raw_variant, uint32_t raw_sample_ct, uint64_t rec_bytes, uint8_t* buf);

// feed(engine, raw file indices in engine order): the caller's genotype-row feeder
// ---- chrX pairs of the r^2 outputs and --clump (ComputeXR2, plink2_ld.cc:7122-7190) ----
// A pair with a chrX variant weighs the male founders down in all six sums -- by 1/2 when both variants are on chrX, by
// 1 - sqrt(2)/2 when one is -- before the same quotient.  Two integer 6-tuples per pair (all founders from `all`, male
// founders from `male`, an engine fed the same rows through a sample map; ldp_pair_stats) are turned from the engines' +-1
// coding and orientation into the reference's counts of the non-major (non-REF) allele -- exactly, in integers -- and
// then the reference's doubles follow, fma for fma (the documented AVX2 build defines FP_FAST_FMA).  Inside chrX the weight
// is dyadic and every sum exact, so WHICH orientation is the target only matters for pairs with an autosome -- but the two
// tuples of a pair must agree on one (each engine picks its major alleles from its own samples).
struct XWeighted {
  ldp_engine* all = nullptr;
  ldp_engine* male = nullptr;             // nullptr: no male founders
  std::vector<uint8_t> is_x;               // per engine row
  std::vector<uint8_t> flip_all, flip_male;  // per engine row: the engine's orientation differs from the target's
  bool unsquared = false;
  struct G {
    int64_t n, g1, q1, g2, q2, d;
  };
  static G counts(const ldp_pair_stats_t& t, bool flip1, bool flip2) {
    G c;
    c.n = t.nm;
    c.g1 = c.n - t.sum1;
    c.q1 = c.n - 2 * static_cast<int64_t>(t.sum1) + t.ssq1;
    c.g2 = c.n - t.sum2;
    c.q2 = c.n - 2 * static_cast<int64_t>(t.sum2) + t.ssq2;
    c.d = c.n - t.sum1 - t.sum2 + t.dot;
    if (flip1) {  // g -> 2 - g
      c.q1 = 4 * c.n - 4 * c.g1 + c.q1;
      c.g1 = 2 * c.n - c.g1;
      c.d = 2 * c.g2 - c.d;
    }
    if (flip2) {
      c.q2 = 4 * c.n - 4 * c.g2 + c.q2;
      c.g2 = 2 * c.n - c.g2;
      c.d = 2 * c.g1 - c.d;
    }
    return c;
  }
  // the reference's doubles from the two count tuples (ComputeXR2 :7160-7185)
  static double weighted(const G& a, const G& m, bool both_x, bool unsquared, double nan_ref) {
    if (!a.n) {
      return nan_ref;
    }
    const double male_downwt = both_x ? 0.5 : (1.0 - 0.5 * 1.4142135623730951);
    const double w_obs = fma(-male_downwt, static_cast<double>(m.n), static_cast<double>(a.n));
    const double w_g1 = fma(-male_downwt, static_cast<double>(m.g1), static_cast<double>(a.g1));
    const double w_g2 = fma(-male_downwt, static_cast<double>(m.g2), static_cast<double>(a.g2));
    const double w_q1 = fma(-male_downwt, static_cast<double>(m.q1), static_cast<double>(a.q1));
    const double w_q2 = fma(-male_downwt, static_cast<double>(m.q2), static_cast<double>(a.q2));
    const double w_d = fma(-male_downwt, static_cast<double>(m.d), static_cast<double>(a.d));
    const double var1 = fma(w_q1, w_obs, -w_g1 * w_g1);
    const double var2 = fma(w_q2, w_obs, -w_g2 * w_g2);
    if (!((var1 > 0.0) && (var2 > 0.0))) {
      return nan_ref;
    }
    const double var_prod = var1 * var2;
    const double cov = fma(w_d, w_obs, -w_g1 * w_g2);
    const double quot = cov * cov / var_prod;
    double r = (1.0 < quot) ? 1.0 : quot;
    if (unsquared) {
      r = sqrt(r);
      if (cov < 0.0) {
        r = -r;
      }
    }
    return r;
  }
  // ---- windowed plans (ldp_set_variants_vcor; --clump): the chrX run [band_first, band_first + band_ct) of the caller's rows, loaded a second time into two
  // ALL-PAIRS engines that hold nothing else (all founders / male founders).  The pairs of a window on chrX then come from the pair kernels and the
  // device-side weighting (ldp_r2_unphased_block_x*: ComputeXR2 as ClumpHighmemR2 and the windowed table call it, plink2_ld.cc:7122-7190, :7343),
  // a chunk of rows at a time, instead of a list of pairs with one wave each.  (A windowed engine has no dense-block plan of its own.)
  ldp_engine* band_all = nullptr;
  ldp_engine* band_male = nullptr;  // nullptr: no male founders
  uint32_t band_first = 0, band_ct = 0;
  std::vector<uint8_t> band_flip_all, band_flip_male;  // per row of the run (empty: none)
  bool band_ready() const { return band_all != nullptr; }
  void band_destroy() {
    if (band_male) {
      ldp_destroy(band_male);
    }
    if (band_all) {
      ldp_destroy(band_all);
    }
    band_all = band_male = nullptr;
  }
  // rows [j, j + R) of the run and the columns their windows reach: R about the window's width, so that the rectangle is about twice the band
  void band_chunk(const uint32_t* lo, uint32_t j, uint32_t j1, uint32_t max_rows, uint32_t* rows, uint32_t* c0) const {
    *c0 = std::max(lo[j], band_first);
    const uint32_t width = j - *c0 + 1;
    *rows = std::min(std::min(j1 - j, max_rows), std::max(512u, std::min(width, 8192u)));
  }
  // f(i, j, value) for every pair lo[j] <= i < j of the rows j in [j0, j1) (inside the run); NaN where the reference's value is undefined
  template <class F>
  void band_dense(const uint32_t* lo, uint32_t j0, uint32_t j1, F f) const {
    const std::vector<uint8_t> ones(band_ct, 1);
    std::vector<double> blk;
    for (uint32_t j = j0; j < j1;) {
      uint32_t rows, c0;
      band_chunk(lo, j, j1, 0xffffffffu, &rows, &c0);
      const uint32_t cols = j + rows - 1 - c0;
      if (cols) {
        blk.assign(static_cast<size_t>(rows) * cols, 0.0);
        if (ldp_r2_unphased_block_x(band_all, band_male, ones.data(), band_flip_all.empty() ? nullptr : band_flip_all.data(), band_flip_male.empty() ? nullptr : band_flip_male.data(),
                                    j - band_first, rows, c0 - band_first, cols, 0, unsquared ? 1 : 0, blk.data(), cols)) {
          die(16, "Error: %s\n", ldp_last_error(band_all));
        }
        for (uint32_t q = 0; q < rows; ++q) {
          for (uint32_t i = std::max(lo[j + q], c0); i < j + q; ++i) {
            f(i, j + q, blk[static_cast<size_t>(q) * cols + (i - c0)]);
          }
        }
      }
      j += rows;
    }
  }
  // ... those with |value| >= min_r2 (NaN never passes), in no particular order
  template <class F>
  void band_hits(const uint32_t* lo, uint32_t j0, uint32_t j1, double min_r2, std::vector<ldp_r2_hit>* buf, F f) const {
    const std::vector<uint8_t> ones(band_ct, 1);
    if (buf->size() < (1u << 20)) {
      buf->resize(1u << 22);
    }
    uint32_t max_rows = 0xffffffffu;
    for (uint32_t j = j0; j < j1;) {
      uint32_t rows, c0;
      band_chunk(lo, j, j1, max_rows, &rows, &c0);
      const uint32_t cols = j + rows - 1 - c0;
      uint64_t found = 0;
      if (cols && ldp_r2_unphased_block_x_hits(band_all, band_male, ones.data(), band_flip_all.empty() ? nullptr : band_flip_all.data(),
                                               band_flip_male.empty() ? nullptr : band_flip_male.data(), j - band_first, rows, c0 - band_first, cols, unsquared ? 1 : 0, min_r2,
                                               buf->data(), buf->size(), &found)) {
        die(16, "Error: %s\n", ldp_last_error(band_all));
      }
      if (found > buf->size()) {  // more passing pairs than the buffer holds: fewer rows per call
        if (rows == 1) {
          die(2, "Error: one chrX variant has more passing partners than the filter buffer holds.\n");
        }
        max_rows = std::max(1u, rows / 2);
        continue;
      }
      for (uint64_t q = 0; q < found; ++q) {
        const uint32_t i = (*buf)[q].first + band_first, jj = (*buf)[q].second + band_first;
        if ((i >= lo[jj]) && (i < jj)) {
          f(i, jj, (*buf)[q].r2);
        }
      }
      j += rows;
    }
  }
  // r^2 (or r) of the listed pairs, each with at least one chrX variant; NaN where the reference's is undefined
  void pairs(const std::vector<uint32_t>& first, const std::vector<uint32_t>& second, std::vector<double>* out) const {
    const size_t n = first.size();
    out->resize(n);
    std::vector<ldp_pair_stats_t> ta, tm;
    double nan_ref;  // (the bits the reference's `0.0 / 0.0` has on x86: sign set)
    {
      const uint64_t bits = 0xfff8000000000000ull;
      memcpy(&nan_ref, &bits, 8);
    }
    for (size_t p0 = 0; p0 < n; p0 += (1u << 21)) {
      const uint32_t cnt = static_cast<uint32_t>(std::min<size_t>(n - p0, 1u << 21));
      ta.resize(cnt);
      tm.assign(cnt, ldp_pair_stats_t{0, 0, 0, 0, 0, 0});
      if (ldp_pair_stats(all, cnt, first.data() + p0, second.data() + p0, ta.data())) {
        die(16, "Error: %s\n", ldp_last_error(all));
      }
      if (male && ldp_pair_stats(male, cnt, first.data() + p0, second.data() + p0, tm.data())) {
        die(16, "Error: %s\n", ldp_last_error(male));
      }
      for (uint32_t q = 0; q < cnt; ++q) {
        const uint32_t i = first[p0 + q], j = second[p0 + q];
        const G a = counts(ta[q], (!flip_all.empty()) && flip_all[i], (!flip_all.empty()) && flip_all[j]);
        const G m = male ? counts(tm[q], (!flip_male.empty()) && flip_male[i], (!flip_male.empty()) && flip_male[j]) : G{0, 0, 0, 0, 0, 0};
        const double r = weighted(a, m, is_x[i] && is_x[j], unsquared, nan_ref);
        (*out)[p0 + q] = r;
      }
    }
  }
};

int chrom_code(const std::string& name_in);
bool chrom_listed(const std::vector<std::string>& terms, const std::string& name);
// The variant-table filters -- chromosome out by --chr / --not-chr / --autosome, --max-alleles, --snps-only, then --extract, then --exclude --
// for every stage of load_inputs(), which builds one (reading the ID files) per call.
struct ChromFacts {
  bool out;   // by --chr / --not-chr / --autosome
  bool zero;  // chromosome 0
  int cls;    // chrom_class()
  int code;   // chrom_code()
};
struct VariantFilter {
  const Args& A;
  const Variants& V;
  const bool by_chrom;  // --chr / --not-chr / --autosome given
  VariantFilter(const Args& args, const Variants& variants);
  // a chromosome name's facts, computed when the name is first asked about
  const ChromFacts& chrom(const std::string& name);
  enum Verdict { kByTable, kByExtract, kByExclude, kPass };  // what drops raw variant v, in the order the reference's log counts survivors
  bool table_passes(uint32_t v) { return (!chrom(V.chrom[v]).out) && (allele_ct_for_filter(V, v) <= A.max_alleles) && !(A.snps_only && V.not_snp[v]); }
  Verdict verdict(uint32_t v) {
    return (!table_passes(v)) ? kByTable
           : (((!A.extract_files.empty()) && !extract_ids_.count(V.id[v])) ? kByExtract : (((!A.exclude_files.empty()) && exclude_ids_.count(V.id[v])) ? kByExclude : kPass));
  }
  bool passes(uint32_t v) { return verdict(v) == kPass; }
  // The raw variants in file order: on_chrom(name, facts) when a chromosome name is first met, before any of its variants is tested -- so a
  // refusal about a chromosome fires even where none of its variants passes, and after a refusal about a variant of an earlier chromosome --,
  // on_variant(v, facts) for every variant that passes.
  template <class OnChrom, class OnVariant>
  void walk(OnChrom on_chrom, OnVariant on_variant) {
    std::unordered_set<const ChromFacts*> met;
    const ChromFacts* cur = nullptr;
    const uint32_t raw_variant_ct = static_cast<uint32_t>(V.id.size());
    for (uint32_t v = 0; v < raw_variant_ct; ++v) {
      const ChromFacts& c = chrom(V.chrom[v]);
      if (&c != cur) {
        cur = &c;
        if (met.insert(cur).second) {
          on_chrom(V.chrom[v], c);
        }
      }
      if (passes(v)) {
        on_variant(v, c);
      }
    }
  }

 private:
  std::unordered_set<std::string> extract_ids_, exclude_ids_;
  std::unordered_map<std::string, ChromFacts> chroms_;
  const std::string* last_name_ = nullptr;  // (the table's chromosomes come in runs: the name and facts last asked about)
  const ChromFacts* last_ = nullptr;
};
// what --clump needs to know about sex chromosomes (ClumpReports :8150-8215, :8460-8482)
struct ClumpSex {
  const std::vector<uint8_t>* vcls = nullptr;  // per included variant: 3 chrX, 4 chrY
  std::vector<uint32_t> male_cols;             // raw sample indices of the male founders
  uint32_t founder_male_ct = 0, founder_female_ct = 0, founder_nosex_ct = 0;
  int prov_storage = 1;                        // ldp_pgen_provisional_ref
  std::vector<uint8_t> prov_bits;
  std::function<void(ldp_engine*, const std::vector<uint32_t>&, const std::vector<uint32_t>*)> feed_cols;
  uint32_t raw_sample_ct = 0;
  // reloads engine row `row` from raw variant `raw`: the main track (aidx < 0) or the copies-of-the-other-alleles row of allele `aidx` of a
  // multiallelic variant; females_missing: the female founders' calls become missing (chrY); mapped: the engine picks its sample columns itself
  std::function<void(ldp_engine*, uint32_t row, uint32_t raw, int32_t aidx, bool females_missing, bool mapped)> allele_row;
};

int clump_reports(const Args& A, const Variants& V, const std::vector<uint32_t>& inc, const std::vector<uint32_t>& chr_idx,
                  const std::vector<uint32_t>& bps, uint32_t founder_ct,
                  const std::function<void(ldp_engine*, const std::vector<uint32_t>&)>& feed, const ClumpSex& SX);

// Everything the commands share: the parsed command line, the variant and sample tables, the open genotype file and the
// included-variant index (chromosome 0 stripped where the reference strips it).  load_inputs() fills it; run_r2() (the
// --r2-unphased outputs and --clump) and run_prune() (--indep-pairwise / --indep-pairphase) consume it.
struct Session {
  double t_begin = 0.0, t_hip_init = 0.0, t_parse = 0.0, t_joined = 0.0;
  Args A;
  Variants V;
  std::thread t_hip;  // HIP runtime start-up, beside the file parsing; joined where the first engine is created, or on the way out
  std::vector<uint8_t> is_founder, sex;  // (a sample --keep / --remove drops is no founder from here on)
  std::vector<uint8_t> sample_kept;      // empty: no sample filter
  uint32_t raw_sample_ct = 0, founder_ct = 0, raw_variant_ct = 0;
  bool is_bed = false;
  std::string gpath;
  ldp_pgen* pg = nullptr;
  int storage_mode = 0, encoding = LDP_GENO_REF, has_multiallelic = 0;
  bool has_dosage = false;  // some record carries a dosage track: --indep-pairwise takes the allele frequencies from them
  // founders' (ref, alt) dosage sums of the variants that have a dosage track (ldp_pgen_dosage_sums), computed once: the
  // frequency filters and the prune's tie-break both want them
  std::unordered_map<uint32_t, std::pair<uint64_t, uint64_t>> dosage_sums;
  void need_dosage_sums(const std::vector<uint32_t>& raw_variants);
  uint64_t rec_bytes = 0;
  const uint8_t* direct_rows = nullptr;  // NULL for variable-width files
  std::vector<uint32_t> inc;             // raw index of every included variant
  std::vector<uint32_t> chr_idx, bps;
  std::vector<uint8_t> vcls;             // per included variant: 0 diploid, 3 chrX, 4 chrY, 5 MT
  uint32_t variant_ct = 0;
  std::vector<uint32_t> mk, xk, yk, tk;  // indices into inc[]: main engine, chrX, chrY, MT under --indep-pairphase
  uint32_t m_ct = 0;
  std::vector<uint32_t> m_chr, m_bps;
  // the count filters (CountFilters): given at all; left to run_prune(), which decides them from the engine's records after the load
  // (then inc[] still holds every variant the table filters leave); otherwise why not, and what the host's pass took
  bool count_filters = false, device_filter = false;
  const char* host_filter_reason = nullptr;
  double host_filter_s = 0.0;
  uint32_t kept_sample_ct = 0;
  std::vector<uint8_t> inc_chr0;  // device_filter: 1 = inc[k] lies on chromosome 0 (empty or shorter than inc: the rest is 0)
  // --mind (the sample-side counterpart).  load_inputs() decides it from a host pass over the rows, or leaves it to run_prune() (mind_device:
  // the counts come from the resident image, ldp_sample_missing_counts; device_filter is set with it, so that every row the table filters leave
  // is loaded under the all-pairs plan first).  A device-side decision that removes samples ends the run with `restart` set and the decision in
  // mind_removed; main() then starts over with a session that has mind_decided set and the same mind_removed, which load_inputs() applies as
  // --remove would have.
  bool mind_device = false, mind_decided = false, restart = false;
  std::vector<uint8_t> mind_removed;     // per sample of the file: 1 = removed by --mind
  uint32_t mind_variant_ct = 0;          // the variants --mind counts over (table filters only: chromosome 0 and multiallelic variants included)
  std::vector<std::string> sample_keys;  // "FID<tab>IID" per sample of the file (kept for <out>.mindrem.id)
  std::vector<std::string> sample_sids;  // SID per sample when the .psam has the column
  bool fid_present = true;
  // the count reports: from the device's records after the load (report_device; device_filter is set with it, as for mind_device), or from the host's
  // pass in load_inputs(), which says why; report_variants: what the reports list (== inc[] when run_prune() writes them)
  bool report_device = false;
  const char* report_host_reason = nullptr;
  // --het: from the resident image after the filters (het_device; device_filter is set with it, as for mind_device), or from the host's pass over
  // the rows of the final variant list, which says why
  bool het_device = false;
  const char* het_host_reason = nullptr;
  std::vector<uint32_t> report_variants;
  // --make-king-table: the pair counts from the resident image after the filters (king_device: the conditions of het_device), or king_host_pass()
  bool king_device = false;
  const char* king_host_reason = nullptr;
  // --hwe / --hardy on the host's pass: seconds spent in ldp_hwe_ln_p_host on the reader's threads, p-values computed, tolerance ties among them
  double hwe_host_s = 0.0;
  uint32_t hwe_host_ct = 0, hwe_host_ties = 0;
  double t_begin_first = 0.0;            // restarted run: main()'s first start (the total of --timing covers both loads)
  // (... and, once the runtime is up, this thread -- the one that creates the engines, their copy threads and their pinned staging -- moves next to the device)
  void join_hip() {
    if (t_hip.joinable()) {
      t_hip.join();
      t_joined = now_s();
      if ((A.gpus <= 1) && !g_dbg.no_bind) {
        bind_near_device(0, &load_affinity);  // (several GPUs: every engine's feeding thread binds itself next to ITS device, p2h_prune.cpp)
      }
    }
  }
  AffinityMask load_affinity;  // what this thread ran on before join_hip() moved it next to device 0: file_to_hbm_done() puts it back
  void file_to_hbm_done() {
    restore_affinity(load_affinity);
    load_affinity.valid = false;
  }
  ~Session() {
    if (t_hip.joinable()) {
      t_hip.join();
    }
  }
};

// --geno / --maf / --max-maf / --mac / --max-mac on one variant's genotype counts, as the reference enforces them (EnforceGenoThresh
// plink2_filter.cc:3498, EnforceFreqConstraints :3791): the one arithmetic both sources of the counts go through -- the host's pass over
// the rows (load_inputs) and the records of the engine's own count pass (run_prune: ldp_get_variant_recs, then ldp_restrict_variants).
struct CountFilters {
  const Args& A;
  bool geno_on, mac_on, freq_on, hwe_on;
  uint32_t missing_max;
  double min_maf, max_maf;
  double hwe_ln_base, hwe_coeff;  // --hwe: a variant with n calls goes when ln p < hwe_ln_base + n * hwe_coeff (EnforceHweThresh, plink2_filter.cc:3539)
  uint32_t geno_removed = 0, hwe_removed = 0, freq_removed = 0;
  uint32_t hwe_min_obs = 0xffffffffu, hwe_max_obs = 0;  // over the variants --hwe computed a p-value for
  CountFilters(const Args& args, uint32_t kept_samples);
  bool any() const { return geno_on || hwe_on || freq_on; }
  bool fails_geno(uint32_t missing) const { return geno_on && (missing > missing_max); }
  // true: the variant goes (and is counted under the filter that removed it), --geno first, then --hwe, then the frequency filters.  missing:
  // calls missing among the kept samples; ref2 / het / alt2: the founders' genotype counts; dosage: their (ref, alt) dosage sums in 16384ths
  // of a copy when the record has a dosage track; hwe_ln_p: ln of the variant's Hardy-Weinberg p-value under --hwe's `midp` setting (from
  // hwe_kernel or ldp_hwe_ln_p_host), nullptr = --hwe does not test the variant (chrY / MT)
  bool drops(uint32_t missing, uint64_t ref2, uint64_t het, uint64_t alt2, const std::pair<uint64_t, uint64_t>* dosage = nullptr, const double* hwe_ln_p = nullptr);
  // the reference's log lines in its order: --geno's, whatever `after_geno` logs (--hardy's report), --hwe's -- with its warning about
  // observation counts, or its error about a threshold too strict for the sample size (exit 7) --, the frequency filters'
  void log_counts(const std::function<void()>& after_geno = nullptr) const;
};
// --hardy: what the one writer takes, whichever pass counted (p2h_reports.cpp)
struct HardyCounts {
  std::vector<uint32_t> variants;            // raw index of every listed variant: what --geno leaves, chrX / chrY / MT apart
  std::vector<uint32_t> hom1, het, hom2;     // the founders' genotype counts (REF/REF, REF/ALT, ALT/ALT)
  std::vector<double> ln_p;                  // under --hardy's `midp` setting
  uint32_t haploid_skipped = 0;              // chrY / MT variants left out (the reference says how many)
  void add(uint32_t v, uint32_t a, uint32_t b, uint32_t c, double lp) {
    variants.push_back(v);
    hom1.push_back(a);
    het.push_back(b);
    hom2.push_back(c);
    ln_p.push_back(lp);
  }
};
void write_hardy(const Session& S, const HardyCounts& H);
// Why a job's count filters cannot be decided from the device's records (nullptr: they can).  The image holds founder columns only and
// --geno counts over the kept samples; one engine holds every row only with one GPU; the r^2 outputs, --clump and --indep-pairphase keep
// the host's pass (their engines are planned before the load); dosage-based frequencies never reach the device.
const char* device_filter_refusal(const Args& A, bool has_dosage, uint32_t kept_samples, uint32_t founder_ct);

// --mind's decision from per-sample missing-call counts (indexed by sample of the file; only kept samples are looked at): MindFilter's integer
// rule, its log lines, <out>.mindrem.id; *removed: per sample of the file.  Returns the number of samples removed.
uint32_t mind_decide(const Session& S, const std::vector<uint32_t>& missing_cts, std::vector<uint8_t>* removed);
// ... applied: the removed samples are neither kept nor founders from here on; exit 13 when nobody is left (plink2.cc:1836-1838)
void mind_apply(Session& S, const std::vector<uint8_t>& removed);

// ---- the count reports (p2h_reports.cpp): --missing (.smiss, .vmiss), --freq (.afreq, .acount), --geno-counts (.gcount) ----
// What the one writer takes, whichever pass counted: the host's over the rows (load_inputs) or the device's count pass (run_prune).
struct ReportCounts {
  std::vector<uint32_t> variants;          // raw index of every listed variant: what the table filters leave, chromosome 0 included
  std::vector<uint32_t> missing;           // per listed variant: missing calls among the kept samples
  std::vector<uint32_t> f_ref2, f_het, f_alt2;  // ... the founders' genotype counts (--freq; meaningless for a variant with several ALT alleles)
  std::vector<uint32_t> s_ref2, s_het, s_alt2;  // ... the kept samples' (--geno-counts); empty: the same samples, the same counts
  std::unordered_map<uint32_t, std::vector<uint32_t>> allele_cts;  // listed variant with several ALT alleles -> the founders' count of every allele
  std::vector<uint32_t> sample_missing;    // per sample of the file (kept samples only are read): missing calls over the listed variants
  uint32_t kept_sample_ct = 0;
};
// the variants the reports list; refuses (exit 63) what the reports do not cover: chrX / chrY / MT, dosage tracks, a phenotype for .smiss, --geno-counts
// with a variant that has several ALT alleles
void reports_list_variants(Session& S, VariantFilter& filter, std::vector<uint32_t>* listed);
// the founders' allele counts of a listed variant with several ALT alleles, from the reader's allele pairs (ldp_pgen_read_alleles): the host
// pass's source, and the device pass's for rows the host built
void reports_count_alleles_host(const Session& S, uint32_t raw_variant, std::vector<uint8_t>* lo, std::vector<uint8_t>* hi, std::vector<uint32_t>* counts);
// the files and their log lines, in the reference's order
void write_reports(const Session& S, const ReportCounts& C);

// ---- --het (p2h_het.cpp): per-sample observed and expected heterozygosity, HetReport (plink2_misc.cc) with its default columns ----
// One variant's expected heterozygosity from the founders' allele counts (cts[0] REF, cts[1 ..] the ALT alleles), as HetThread forms it:
// from the frequencies (count * (1 / total); nothing observed: 1 / alleles each) or, small_sample, from the counts.  false: the reference
// skips the variant and counts it in its "monomorphic" warning.
bool het_expected(const uint32_t* cts, uint32_t allele_ct, bool small_sample, double* ehet);
// het_all_missing_skipped: one more variant the reference skips and counts as monomorphic.  A variable-width .pgen stores a variant nobody has a
// call at as an empty list of exceptions from "missing", and HetThread's branch for such records (plink2_misc.cc:9952-9956) skips it, while
// the same variant in a .bed or a fixed-width .pgen counts with the frequency 1/2 of an unobserved allele and changes no sample's figures
// (everybody misses it).  Both passes apply it where the file is variable-width (Session::direct_rows is NULL), the variant has one ALT allele
// (the others are read in full, PgrGetM) and every kept sample misses the call.
// What both sources of the per-sample sums go through -- the device's pass over the resident image (run_prune: ldp_sample_het_counts) and the
// host's pass over the rows (het_host_pass) --, so that the two write the same bytes.  With m kept variants every ehet_v becomes the integer
// q_v = llrint(ehet_v * 2^k), k = min(52, 62 - bit_length(m)); a sample's expected count is (sum of all q_v - sum of the q_v of the variants
// it misses) * 2^-k: integer sums, the same in any order.
struct HetPlan {
  int k = 52;
  uint64_t total = 0;              // sum of q_v over the kept variants
  uint32_t kept = 0, skipped = 0;  // variants that count / that HetThread skips as monomorphic
  std::vector<uint64_t> weight;    // per variant of the list: q_v, 0 for a skipped one
  std::vector<uint8_t> include;    // per variant of the list: 1 = kept
  // ehet: per variant of the list; ok: het_expected()'s answer for it
  void build(const std::vector<double>& ehet, const std::vector<uint8_t>& ok);
};
// per sample of the file (kept samples only are read): het calls, missing calls and the summed q_v of the missing calls over the kept variants
struct HetSums {
  std::vector<uint32_t> het_ct, missing_ct;
  std::vector<uint64_t> missing_weight;
};
// the reference's warning about skipped variants, <out>.het[.zst] and its log line
void het_write(const Session& S, const HetPlan& plan, const HetSums& sums);
// the log lines and errors HetReport has before it reads a genotype ('--het small-sample' without founders, non-autosomal variants excluded, none left);
// non_autosomal: variants of the final list on chrX / chrY / MT, autosomal: the others
void het_preamble(const Session& S, uint32_t autosomal, uint32_t non_autosomal);
// the host's pass: the autosomal variants of the final list (S.inc), every kept sample; p2h_inputs.cpp, beside the other passes over the rows
void het_host_pass(Session& S);

// ---- --make-king-table (p2h_king.cpp): the KING-robust table, CalcKing (plink2_matrix_calc.cc:1662-2460) ----
// The one writer both sources of the counts go through: the device's (run_prune: ldp_king_counts_block / ldp_king_block_hits) and the host's
// pass (king_host_pass).  Lines come row ascending, column ascending; row and col index the kept samples in file order, the line's first
// sample being the later one.
class KingWriter {
 public:
  explicit KingWriter(const Session& S);
  // one pair: the kinship is formed here from the integers (ComputeKinship), the filter applied, the line appended
  void pair(uint32_t row, uint32_t col, const ldp_king_counts_t& c);
  // pairs the device's hit form left out: they count as filtered
  void add_filtered(uint64_t n) { filtered_ += n; }
  // closes the file, writes <out>.kin0.id where 'id' is not among the columns, and logs what the reference logs; variant_ct: variants processed
  void finish(uint32_t variant_ct);

 private:
  const Session& S_;
  std::vector<uint32_t> kept_;  // sample of the file per kept sample
  std::vector<std::string> ids_;  // the ID columns of every kept sample, tab-terminated
  bool col_fid_ = false, col_sid_ = false;
  OutFile f_;
  std::string path_, buf_;
  uint64_t filtered_ = 0, pairs_ = 0;
};
// the log lines and errors CalcKing has before it reads a genotype (fewer than two samples; non-autosomal variants excluded, none left)
void king_preamble(const Session& S, uint32_t sample_ct, uint32_t autosomal, uint32_t non_autosomal);
// The host's popcount pass over sample-major bit-planes (words per sample: het, hom, hom-ALT over the variants): every pair in the table's order
// through the writer, on `nthreads` threads
void king_pairs_host(const std::vector<uint64_t>& het, const std::vector<uint64_t>& hom, const std::vector<uint64_t>& alt, size_t words, uint32_t sample_ct, uint32_t nthreads,
                     KingWriter* w);
// the host's pass: main-track rows of the autosomal variants of the final list (S.inc), every kept sample; p2h_inputs.cpp, beside the other passes over the rows
void king_host_pass(Session& S);
void logprintf_ww(const char* fmt, ...);  // logprintf with the reference's word wrap at 79 columns (logprintfww)

void load_inputs(Session& S, int argc, char** argv);
int run_r2(Session& S);
int run_prune(Session& S);

}  // namespace p2h
#endif
