// p2h_prune.cpp -- plink2-hip: --indep-pairwise / --indep-pairphase (one translation unit of the front-end; plink2_hip_cli.cpp has the overview)
#include "p2h_cli.h"

namespace p2h {

namespace {

// one bit per sample of the file (bit s & 7 of byte s >> 3), set where keep(s)
template <class Keep>
std::vector<uint8_t> sample_mask(uint32_t raw_sample_ct, Keep keep) {
  std::vector<uint8_t> mask((static_cast<size_t>(raw_sample_ct) + 7) / 8, 0);
  for (uint32_t s = 0; s < raw_sample_ct; ++s) {
    if (keep(s)) {
      mask[s >> 3] |= static_cast<uint8_t>(1u << (s & 7));
    }
  }
  return mask;
}

// x = min(x, v)
void atomic_min(std::atomic<uint32_t>* x, uint32_t v) {
  uint32_t cur = x->load();
  while ((v < cur) && !x->compare_exchange_weak(cur, v)) {
  }
}

double gb_per_s(double bytes, double seconds) { return (seconds > 0.0) ? (bytes / 1e9 / seconds) : 0.0; }

}  // namespace

// ---- --indep-pairwise / --indep-pairphase ----
void Session::need_dosage_sums(const std::vector<uint32_t>& raw_variants) {
  std::vector<uint32_t> todo;
  for (uint32_t v : raw_variants) {
    if (!dosage_sums.count(v)) {
      todo.push_back(v);
    }
  }
  if (todo.empty()) {
    return;
  }
  const std::vector<uint8_t> founder_mask = sample_mask(raw_sample_ct, [&](uint32_t s) { return is_founder[s] != 0; });
  const uint8_t* mask = (founder_ct == raw_sample_ct) ? nullptr : founder_mask.data();
  std::vector<std::pair<uint64_t, uint64_t>> out(todo.size());
  std::atomic<uint32_t> next(0);
  std::atomic<int> bad(0);
  auto worker = [&]() {
    for (uint32_t t = next.fetch_add(64); (t < todo.size()) && !bad.load(); t = next.fetch_add(64)) {
      for (uint32_t q = t; q < std::min<size_t>(todo.size(), t + 64); ++q) {
        if (ldp_pgen_dosage_sums(pg, todo[q], mask, &out[q].first, &out[q].second)) {
          bad.store(1);
          return;
        }
      }
    }
  };
  const uint32_t nthreads = std::max<uint32_t>(1, std::min<uint32_t>({64u, std::thread::hardware_concurrency(), static_cast<uint32_t>((todo.size() + 63) / 64)}));
  std::vector<std::thread> pool;
  for (uint32_t t = 1; t < nthreads; ++t) {
    pool.emplace_back(worker);
  }
  worker();
  for (std::thread& t : pool) {
    t.join();
  }
  if (bad.load()) {
    die(6, "\nError: %s: %s\n", gpath.c_str(), ldp_pgen_last_error(pg));
  }
  for (size_t q = 0; q < todo.size(); ++q) {
    dosage_sums[todo[q]] = out[q];
  }
}

// --indep-pairwise / --indep-pairphase: one run, phase by phase in the order run() calls them (LdPrune, plink2_ld.cc:2530-2720;
// IndepPairwise / IndepPairphase :1284-1450, :2020-2330; LdPruneWrite :2464-2528).  The members are what the phases share.
struct PruneJob {
  Session& S;
  const Args& A = S.A;
  const Variants& V = S.V;
  const double t_begin;
  const std::vector<uint8_t>& is_founder = S.is_founder;
  const std::vector<uint8_t>& sex = S.sex;
  const uint32_t raw_sample_ct = S.raw_sample_ct, founder_ct = S.founder_ct, raw_variant_ct = S.raw_variant_ct;
  const std::string& gpath = S.gpath;
  ldp_pgen* const pg = S.pg;
  const int storage_mode = S.storage_mode, encoding = S.encoding, has_multiallelic = S.has_multiallelic;
  const uint64_t rec_bytes = S.rec_bytes;
  const uint8_t* const direct_rows = S.direct_rows;
  const std::vector<uint32_t>&inc = S.inc, &chr_idx = S.chr_idx, &bps = S.bps;
  const std::vector<uint8_t>& vcls = S.vcls;
  uint32_t variant_ct = S.variant_ct, m_ct = S.m_ct;  // (filter_on_device() shrinks them together with the session's variant tables)
  const std::vector<uint32_t>&mk = S.mk, &xk = S.xk, &yk = S.yk, &tk = S.tk, &m_chr = S.m_chr, &m_bps = S.m_bps;
  const double &t_hip_init = S.t_hip_init, &t_parse = S.t_parse, &t_joined = S.t_joined;

  ldp_params P;
  bool duplicate_ids = false;
  double t_tables_done = 0, t_planned = 0, t_load0 = 0, t_load1 = 0, t_run1 = 0;
  double t_rows0 = 0, t_rows1 = 0;  // load_diploid_rows(): the file -> HBM leg itself
  // the count filters decided from the engine's records (Session::device_filter)
  uint64_t filter_rows_compacted = 0, filter_rows_bounced = 0;
  double filter_ms_compact = 0.0, filter_s = 0.0, filter_ms_recount = 0.0;
  // --hwe / --hardy from the same records (filter_on_device): p-values computed, hwe_kernel's time, variants whose flag byte names a tolerance tie
  double hwe_ms_kernel = 0.0;
  uint64_t hwe_pvals = 0;
  uint32_t hwe_ties = 0;
  int world = 1, n_devices = 1;
  bool alias_devices = false;
  std::vector<ldp_engine*> eng;
  uint32_t subcontig_ct = 0;
  std::vector<uint32_t> sub_info, sub_owner;  // several engines: (length, first variant) and owning engine of every subcontig
  std::vector<uint64_t> removed;    // bit k: variant k (include order) is pruned
  std::vector<uint64_t> preferred;  // --indep-preferred, same indexing; empty: none
  std::vector<uint8_t> founder_mask;
  std::vector<uint32_t> founder_idx;
  // geometry of the rows on their way to the engines (set_row_geometry)
  bool all_founders = false;
  uint64_t in_rec = 0, in_phase_off = 0, out_rec = 0, direct_off = 0;
  int load_encoding = 0, direct_fd = -1;
  const uint8_t* direct = nullptr;
  // what the bulk load leaves for the host-built rows
  bool device_multi = false;
  uint32_t pending_unphased = UINT32_MAX;

  explicit PruneJob(Session& s) : S(s), t_begin(s.t_begin) {}

  [[noreturn]] void die_unphased(uint32_t raw_v) const {
    die(7, "\nError: --indep-pairphase: 0-based variant #%u is not fully phased.\n", raw_v);  // plink2_ld.cc:2047
  }
  // a library call that has to succeed: otherwise the engine's message and exit 16
  static void must(ldp_engine* e, int rc) {
    if (rc) {
      die(16, "\nError: %s\n", ldp_last_error(e));
    }
  }
  // all m_ct records of an engine
  std::vector<ldp_variant_rec> recs_of(ldp_engine* e) const {
    std::vector<ldp_variant_rec> recs(std::max<uint32_t>(m_ct, 1));
    must(e, ldp_get_variant_recs(e, 0, m_ct, recs.data()));
    return recs;
  }
  // per-column values of the image into file sample order (column f of the image is founder f of the file: every kept sample is a founder here)
  template <class T>
  void to_file_order(const std::vector<T>& by_column, std::vector<T>* per_sample) const {
    per_sample->assign(raw_sample_ct, 0);
    for (uint32_t f = 0; f < founder_ct; ++f) {
      (*per_sample)[founder_idx[f]] = by_column[f];
    }
  }
  // --indep-preferred bits of a subset of the variants (ks: include-order indices, in the subset's engine order)
  std::vector<uint64_t> sub_preferred(const std::vector<uint32_t>& ks) const {
      std::vector<uint64_t> out;
      if (!preferred.empty()) {
        out.assign((ks.size() + 63) / 64 + 1, 0);
        for (size_t q = 0; q < ks.size(); ++q) {
          if ((preferred[ks[q] >> 6] >> (ks[q] & 63)) & 1) {
            out[q >> 6] |= 1ull << (q & 63);
          }
        }
      }
      return out;
  }
  // an engine's removed bits (its own variant order) into the run's bitmap
  void scatter(const std::vector<uint64_t>& bm, const std::vector<uint32_t>& ks) {
      for (size_t q = 0; q < ks.size(); ++q) {
        if ((bm[q >> 6] >> (q & 63)) & 1) {
          removed[ks[q] >> 6] |= 1ull << (ks[q] & 63);
        }
      }
  }

  void set_params() {
    memset(&P, 0, sizeof(P));
    P.founder_ct = A.pairphase ? 2 * founder_ct : founder_ct;  // --indep-pairphase: haplotypes (plink2_ld.cc:1506)
    P.prune_window_size = A.window;
    P.prune_window_incr = A.step;
    P.window_is_bp = A.window_is_bp;
    P.plink1_order = (A.order == 1);
    P.prune_last_param = A.r2;
    if (!A.have_prune) {  // a run of reports alone: rows, count pass and records under the all-pairs plan, no window is ever used
      P.prune_window_size = 2;
      P.prune_window_incr = 1;
      P.window_is_bp = 0;
      P.prune_last_param = 0.5;
    }
  }

  // --dry-run: the plan only (no device)
  int dry_run() {
    ldp_engine* e = nullptr;
    P.device = -1;
    S.join_hip();
    const double t_plan0 = now_s();
    if (ldp_create(&P, &e) || ldp_set_variants(e, m_ct, m_chr.data(), A.window_is_bp ? m_bps.data() : nullptr)) {
      die(16, "Error: planning failed.\n");
    }
    if (A.timing) {
      logprintf("[timing] table parse %.3f s, joined at %.3f s, variant table passes %.3f s, engine plan %.3f s\n", t_parse, t_joined - t_begin,
                t_plan0 - t_joined, now_s() - t_plan0);
    }
    uint32_t sct = 0;
    uint64_t cand = 0;
    ldp_get_subcontigs(e, &sct, nullptr, 0);
    ldp_get_band(e, nullptr, &cand);
    logprintf("dry-run: founders=%u variants=%u window=%u step=%u window_is_bp=%d r2=%a order=%d subcontigs=%u candidate_pairs=%llu\n",
              founder_ct, m_ct, A.window, A.step, A.window_is_bp ? 1 : 0, A.r2, A.order, sct, static_cast<unsigned long long>(cand));
    if (!xk.empty() || !yk.empty() || !tk.empty()) {
      logprintf("dry-run: chrX variants=%zu chrY variants=%zu%s (separate engines)\n", xk.size(), yk.size(), tk.empty() ? "" : " + MT");
    }
    ldp_destroy(e);
    return 0;
  }

  // unique IDs (plink2_ld.cc:2573-2592): checked here, beside the HIP start-up, reported where the reference does
  void check_unique_ids() {
    {
      // open-addressing table of variant indices keyed by a 64-bit FNV-1a hash of the ID
      uint32_t bits = 4;
      while ((1ull << bits) < 2ull * variant_ct) {
        ++bits;
      }
      const uint64_t mask = (1ull << bits) - 1;
      std::vector<uint32_t> table(static_cast<size_t>(1) << bits, 0xffffffffu);
      for (uint32_t k = 0; (k < variant_ct) && !duplicate_ids; ++k) {
        const std::string& id = V.id[inc[k]];
        uint64_t h = 0xcbf29ce484222325ull;
        for (unsigned char ch : id) {
          h = (h ^ ch) * 0x100000001b3ull;
        }
        uint64_t slot = (h ^ (h >> 29)) & mask;
        while (table[slot] != 0xffffffffu) {
          if (V.id[inc[table[slot]]] == id) {
            duplicate_ids = true;
            break;
          }
          slot = (slot + 1) & mask;
        }
        table[slot] = k;
      }
    }
  }

  // One GPU: the engine is created and planned (host work: ldp_create binds the device lazily) while the HIP runtime
  // is still starting; several GPUs: the device count decides how many engines there are, so wait for it first.
  void plan_engines() {
    if (A.gpus > 1) {
      S.join_hip();
      const int ndev = ldp_device_count();
      if (ndev < 1) {
        die(16, "Error: no usable HIP device (plink2-hip has no CPU compute path).\n");
      }
      // --debug-alias-devices (tests, one-GPU boxes): as many engines as --gpus asks for, dealt round-robin onto the devices
      // there are -- every host-side step of the N-device run (shard plan, per-engine loads, one thread per engine, segment pack /
      // exchange / stitch) then runs on a single device; RCCL refuses a device twice, so the exchange is the host transport.
      alias_devices = g_dbg.alias_devices;
      n_devices = ndev;
      world = alias_devices ? A.gpus : std::min(A.gpus, ndev);
    }
    eng.assign(world, nullptr);
    for (int r = 0; r < world; ++r) {
      P.device = r % n_devices;
      int rc = ldp_create(&P, &eng[r]);
      if (rc) {
        die(16, "Error: ldp_create failed (%d).\n", rc);
      }
      // (count filters from the device's records: rows, count pass and records first, no band -- filter_on_device() plans)
      rc = S.device_filter ? ldp_set_variants_matrix(eng[r], m_ct) : ldp_set_variants(eng[r], m_ct, m_chr.data(), A.window_is_bp ? m_bps.data() : nullptr);
      if (rc) {
        die(16, "Error: %s\n", ldp_last_error(eng[r]));
      }
      ldp_get_subcontigs(eng[r], &subcontig_ct, nullptr, 0);
      if (world > 1) {
        if (r == 0) {
          sub_info.assign(2 * static_cast<size_t>(subcontig_ct), 0);
          sub_owner.assign(subcontig_ct, 0);
          ldp_get_subcontigs(eng[r], &subcontig_ct, sub_info.data(), subcontig_ct);
        }
        rc = ldp_set_shard(eng[r], r, world, (r == 0) ? sub_owner.data() : nullptr);
        if (rc) {
          die(16, "Error: %s\n", ldp_last_error(eng[r]));
        }
      }
    }
  }

  void check_before_loading() {
    if (duplicate_ids) {  // plink2_ld.cc:2590-2592
      die(7, "Error: --indep-pair%s requires unique variant IDs. (--set-all-var-ids and/or --rm-dup may help.)\n", A.pairphase ? "phase" : "wise");
    }
    if (S.has_dosage) {
      // chrX / chrY / MT: the reference's dosage-aware counts weigh males and females differently there (plink2_data.cc:2467-2620)
      for (const std::vector<uint32_t>* ks : {&xk, &yk, &tk}) {
        for (uint32_t k : *ks) {
          if (ldp_pgen_variant_has_dosage(pg, inc[k])) {
            die(63, "Error: variant '%s' on a sex chromosome or chrM has dosages, which plink2-hip reads on the autosomes only.\n", V.id[inc[k]].c_str());
          }
        }
      }
    }
  }

  // --indep-preferred (plink2_ld.cc:2594-2640)
  void read_preferred() {
    if (!A.preferred.empty()) {
      std::unordered_set<std::string> want;
      std::ifstream pin(A.preferred);
      if (!pin) {
        die(3, "Error: Failed to open %s.\n", A.preferred.c_str());
      }
      std::string tok;
      while (pin >> tok) {
        want.insert(tok);
      }
      preferred.assign((static_cast<size_t>(variant_ct) + 63) / 64, 0);
      uint32_t ct = 0;
      for (uint32_t k = 0; k < variant_ct; ++k) {
        if (want.count(V.id[inc[k]])) {
          preferred[k >> 6] |= 1ull << (k & 63);
          ++ct;
        }
      }
      logprintf("--indep-preferred: %u variant%s loaded.\n", ct, ct == 1 ? "" : "s");
    }
  }

  // ---- genotype rows of the diploid (+MT) variants -> engines, straight from the mapping (or the decoder's buffers);
  // the founder columns (CopyNyparrNonemptySubset, pgenlib_misc.cc:32,185) are picked on the device.
  void set_row_geometry() {
    all_founders = (founder_ct == raw_sample_ct);
    // --indep-pairphase rows: 2-bit codes, padding to a dword, phaseinfo bits (LDP_GENO_PHASED, ldprune_hip.h)
    in_rec = A.pairphase ? ldp_phased_row_bytes(2 * raw_sample_ct) : rec_bytes;
    in_phase_off = ldp_phased_phase_offset(2 * raw_sample_ct);
    out_rec = A.pairphase ? ldp_phased_row_bytes(2 * founder_ct) : ((static_cast<uint64_t>(founder_ct) + 3) / 4);
    load_encoding = A.pairphase ? (LDP_GENO_REF | LDP_GENO_PHASED) : encoding;
    direct = A.pairphase ? nullptr : direct_rows;  // phased rows always come through the decoder
    direct_off = 0;
    // Fixed-width rows go from the file to the engine's pinned ring with pread() (ldp_load_genotypes_fd), not by memcpy out of the
    // mapping: a 12 GB mapping is faulted in page run by page run, and what that costs swung between 0.35 and 0.97 s from one run to
    // the next on the same host, while 32 readers take 0.36-0.38 s every time (--debug-load-map: the mapping)
    direct_fd = (direct && !g_dbg.load_map) ? ldp_pgen_direct_fd(pg, &direct_off, nullptr) : -1;
    founder_mask = sample_mask(raw_sample_ct, [&](uint32_t s) { return is_founder[s] != 0; });
    founder_idx.clear();
    for (uint32_t s = 0; s < raw_sample_ct; ++s) {
      if (is_founder[s]) {
        founder_idx.push_back(s);
      }
    }
  }

  // the diploid (+MT) variants' rows, file -> engines (the loop of IndepPairwise, plink2_ld.cc:1345-1390)
  void load_diploid_rows() {
    // Chunks of ~256 MiB of decoded rows.  Variable-width .pgen: the next chunk is decoded (all host threads, see
    // ldp_pgen_read) while the engine takes the current one, two buffers alternating; small enough that the
    // buffers' first-touch page faults are paid once, large enough for ~60 decode tasks per chunk.
    const uint32_t kChunk = std::max<uint32_t>(1, static_cast<uint32_t>((direct ? (1024ull << 20) : (256ull << 20)) / std::max<uint64_t>(in_rec, 1)));
    // two buffers of one chunk each, malloc'ed (a vector would zero-fill them on this thread: 2 x 256 MiB of page faults and
    // memset before the first record is decoded; this way the decoder's threads touch the pages first, in parallel) and
    // never freed: returning ~0.5 GiB of touched pages to the kernel costs tens of ms and the process exits soon
    uint8_t* decoded[2] = {nullptr, nullptr};
    std::vector<uint8_t> gather;
    // the runs (maximal stretches of included variants that are contiguous in the file, capped at kChunk)
    struct Run {
      uint32_t q, raw0, n;
    };
    std::vector<Run> runs;
    for (uint32_t q = 0; q < m_ct;) {
      const uint32_t raw0 = inc[mk[q]];
      uint32_t run = 1;
      while (q + run < m_ct && inc[mk[q + run]] == raw0 + run && run < kChunk) {
        ++run;
      }
      runs.push_back({q, raw0, run});
      q += run;
    }
    // Non-founders in the file: the engines pick the founder columns themselves while converting (ldp_set_sample_map), so the
    // rows go up as the file has them.  (--indep-pairphase rows carry phase bits the gather does not move: host subset.)
    const bool device_subset = (!all_founders) && !A.pairphase;
    if (device_subset) {
      for (int r = 0; r < world; ++r) {
        must(eng[r], ldp_set_sample_map(eng[r], raw_sample_ct, founder_idx.data(), nullptr));
      }
    }
    // Variable-width records are decoded ON THE DEVICE from the file's own bytes (ldp_load_pgen_records: main track of every
    // record type, LD-compressed chains, and -- when the engine's samples are the file's -- the collapse of variants with more
    // than one ALT allele); --indep-pairphase rows (phase track) and --debug-host-decode take the host decoder below.
    // --indep-pairphase: main AND phase track on the device (ldp_load_pgen_records_phased) when every sample is a founder -- variants with
    // more than one ALT allele included since round 5 (collapse and phase bits in one kernel); otherwise the host decoder.
    const bool device_phase = A.pairphase && all_founders && (storage_mode != 0x01) && (storage_mode != 0x02) && (!g_dbg.host_decode);
    const bool device_decode = (!direct) && ((!A.pairphase) || device_phase) && (storage_mode != 0x01) && (storage_mode != 0x02) && (!g_dbg.host_decode);
    // (records with several ALT alleles are collapsed on the device as well: over the file's samples, or over the founders when the
    // engines pick those through a subset sample map)
    device_multi = device_decode && (all_founders || device_subset);
    uint64_t file_size = 0;
    const void* file_bytes = device_decode ? ldp_pgen_file_bytes(pg, &file_size) : nullptr;
    // What the device decoder wants of a run: its record index, the record an LD-compressed chain starts from when that lies in front of the
    // run, and the allele count of every record that is to be collapsed.  0, or the exit code with its message (a feeding thread must not die).
    struct RunIndex {
      std::vector<ldp_pgen_rec> recs;
      uint32_t base_v = UINT32_MAX;
      ldp_pgen_rec base_rec;
      const ldp_pgen_rec* base() const { return (base_v != UINT32_MAX) ? &base_rec : nullptr; }
    };
    auto index_run = [&](const Run& rn, RunIndex* ix, std::string* err) -> int {
      ix->recs.resize(rn.n);
      ix->base_v = UINT32_MAX;
      if (ldp_pgen_record_index(pg, rn.raw0, rn.n, ix->recs.data(), &ix->base_v) || ((ix->base_v != UINT32_MAX) && ldp_pgen_record_index(pg, ix->base_v, 1, &ix->base_rec, nullptr))) {
        *err = gpath + ": malformed variant record index.";
        return 6;
      }
      for (uint32_t t = 0; device_multi && (t < rn.n); ++t) {
        const uint32_t alts = V.alt_ct[rn.raw0 + t];
        if ((alts > 1) && (vcls[mk[rn.q + t]] != 5)) {
          if (alts > 254) {
            *err = "variant '" + V.id[rn.raw0 + t] + "' has more than 254 ALT alleles: not supported by plink2-hip.";
            return 63;
          }
          ix->recs[t].allele_ct = static_cast<uint8_t>(alts + 1);
        }
      }
      return 0;
    };
    // Rows of a run to an engine.  Fixed-width rows as the file has them go with pread() straight into the engine's pinned ring
    // (ldp_load_genotypes_fd); decoded or gathered rows, and the mapping under --debug-load-map, from memory.  The library's return code.
    auto load_rows = [&](ldp_engine* e, const Run& rn, const uint8_t* src, uint64_t stride) -> int {
      const int enc = load_encoding | (device_subset ? LDP_GENO_MAPPED : 0);
      const uint64_t file_off = static_cast<uint64_t>(rn.raw0) * rec_bytes;
      const bool from_fd = direct && (src == direct + file_off) && (direct_fd >= 0);
      return from_fd ? ldp_load_genotypes_fd(e, rn.q, rn.n, direct_fd, direct_off + file_off, stride, enc) : ldp_load_genotypes(e, rn.q, rn.n, src, stride, LDP_MEM_HOST, enc);
    };
    RunIndex rec_index;
    std::thread decoder;
    // The decoder runs beside the engine's copy threads (ldp_load_genotypes: 16 of them feeding the pinned ring); a record
    // takes microseconds, so a few dozen threads keep ahead of PCIe and more only get in the copies' way.
    const uint32_t decode_threads = g_dbg.decode_threads ? g_dbg.decode_threads : 32;
    double t_wait_decode = 0.0, t_load_calls = 0.0;
    // Several engines: each is fed by a host thread of its own, all at once -- the reference's main thread fills EVERY worker's slot of a
    // batch and the workers run together (plink2_ld.cc:1292-1417).  A feeding thread walks only the file ranges of its engine's shard,
    // binds itself next to ITS device (NUMA node of the device's PCI function) and gives the engine copy threads and a pinned ring of
    // its own there (ldp_use_private_copy_threads), so N PCIe links work at a time instead of one.  (Rows that reach the engines through
    // the host decoder or the host-side founder subset keep the one-after-the-other loop below: --indep-pairphase, --debug-host-decode.)
    if ((world > 1) && (!A.pairphase) && (!g_dbg.serial_feed) && (direct || device_decode) && (all_founders || device_subset)) {
      struct FeedStat {
        double t0 = -1.0, t1 = -1.0;
        uint64_t rows = 0, calls = 0;
        int node = -1, rc = 0;
        std::string err;
      };
      std::vector<FeedStat> stat(world);
      // variant ranges [first, end) of every engine's subcontigs, in variant order
      std::vector<std::vector<std::pair<uint32_t, uint32_t>>> mine(world);
      for (uint32_t s = 0; s < subcontig_ct; ++s) {
        mine[sub_owner[s]].push_back({sub_info[2 * s + 1], sub_info[2 * s + 1] + sub_info[2 * s]});
      }
      for (auto& v : mine) {
        std::sort(v.begin(), v.end());
      }
      std::vector<std::thread> feeders;
      for (int r = 0; r < world; ++r) {
        feeders.emplace_back([&, r]() {
          FeedStat& st = stat[r];
          AffinityMask before;
          if (!g_dbg.no_bind) {
            st.node = bind_near_device(r % n_devices, &before);
          }
          (void)ldp_use_private_copy_threads(eng[r]);
          RunIndex idx;
          size_t at = 0;  // first range of mine[r] that may still reach the current run
          for (const Run& rn : runs) {
            while ((at < mine[r].size()) && (mine[r][at].second <= rn.q)) {
              ++at;
            }
            uint64_t owned_rows = 0;
            for (size_t k = at; (k < mine[r].size()) && (mine[r][k].first < rn.q + rn.n); ++k) {
              owned_rows += std::min(mine[r][k].second, rn.q + rn.n) - std::max(mine[r][k].first, rn.q);
            }
            if (!owned_rows) {
              continue;  // another engine's part of the file
            }
            const double tc = now_s();
            if (st.t0 < 0.0) {
              st.t0 = tc;
            }
            if (device_decode) {
              st.rc = index_run(rn, &idx, &st.err);
              if (st.rc) {
                return;
              }
              const int rc = ldp_load_pgen_records(eng[r], rn.q, rn.n, file_bytes, file_size, LDP_MEM_HOST, idx.recs.data(), idx.base(), raw_sample_ct, nullptr);
              if (rc) {
                st.rc = (rc == LDP_ERR_INVALID) ? 6 : 16;
                st.err = gpath + ": " + ldp_last_error(eng[r]);
                return;
              }
            } else if (load_rows(eng[r], rn, direct + static_cast<uint64_t>(rn.raw0) * rec_bytes, in_rec)) {
              st.rc = 16;
              st.err = ldp_last_error(eng[r]);
              return;
            }
            st.t1 = now_s();
            st.rows += owned_rows;
            ++st.calls;
          }
          restore_affinity(before);
        });
      }
      for (std::thread& t : feeders) {
        t.join();
      }
      for (int r = 0; r < world; ++r) {
        if (stat[r].rc) {
          die(stat[r].rc, "\nError: %s\n", stat[r].err.c_str());
        }
      }
      if (A.timing) {
        // the engines' load intervals (seconds since main()): they overlap when the engines are fed at the same time
        double busy_sum = 0.0, span0 = 1e300, span1 = 0.0;
        for (int r = 0; r < world; ++r) {
          const FeedStat& st = stat[r];
          if (st.t0 < 0.0) {
            logprintf("\n[timing] engine %d (device %d): no rows of its own in this file", r, r % n_devices);
            continue;
          }
          logprintf("\n[timing] engine %d (device %d, NUMA node %d): fed %.3f - %.3f s (%.3f s), %llu rows in %llu calls, %.1f GB/s", r, r % n_devices, st.node,
                    st.t0 - t_begin, st.t1 - t_begin, st.t1 - st.t0, static_cast<unsigned long long>(st.rows), static_cast<unsigned long long>(st.calls),
                    gb_per_s(static_cast<double>(st.rows) * static_cast<double>(direct ? rec_bytes : out_rec), st.t1 - st.t0));
          busy_sum += st.t1 - st.t0;
          span0 = std::min(span0, st.t0);
          span1 = std::max(span1, st.t1);
        }
        if (span1 > span0) {
          logprintf("\n[timing] %d engines fed concurrently: load span %.3f s, sum of the engines' own intervals %.3f s (overlap factor %.2f)\n", world, span1 - span0, busy_sum,
                    busy_sum / (span1 - span0));
        }
      }
      return;
    }
    int decode_rc = 0;
    uint32_t unphased_at = 0;
    pending_unphased = UINT32_MAX;
    auto start_decode = [&](size_t k) {
      if (direct || device_decode || k >= runs.size()) {
        return;
      }
      if (!decoded[k & 1]) {
        uint32_t longest = 0;
        for (const Run& rn : runs) {
          longest = std::max(longest, rn.n);
        }
        decoded[k & 1] = static_cast<uint8_t*>(malloc(static_cast<size_t>(longest) * in_rec + 64));
        if (!decoded[k & 1]) {
          die(2, "\nError: Out of memory.\n");
        }
      }
      decoder = std::thread([&, k]() {
        decode_rc = A.pairphase ? ldp_pgen_read_phased(pg, runs[k].raw0, runs[k].n, decoded[k & 1], in_rec, founder_mask.data(), decode_threads, &unphased_at)
                                : ldp_pgen_read(pg, runs[k].raw0, runs[k].n, decoded[k & 1], rec_bytes, decode_threads);
      });
    };
    start_decode(0);
    for (size_t k = 0; k < runs.size(); ++k) {
      const uint32_t q = runs[k].q;
      const uint32_t raw0 = runs[k].raw0;
      const uint32_t run = runs[k].n;
      const uint8_t* src;
      uint64_t stride = in_rec;
      if (device_decode) {
        std::string err;
        if (const int code = index_run(runs[k], &rec_index, &err)) {
          die(code, "\nError: %s\n", err.c_str());
        }
        const double tl0 = now_s();
        for (int r = 0; r < world; ++r) {
          uint32_t bad_q = UINT32_MAX;
          const int rc = device_phase ? ldp_load_pgen_records_phased(eng[r], q, run, file_bytes, file_size, LDP_MEM_HOST, rec_index.recs.data(), rec_index.base(), raw_sample_ct, &bad_q)
                                      : ldp_load_pgen_records(eng[r], q, run, file_bytes, file_size, LDP_MEM_HOST, rec_index.recs.data(), rec_index.base(), raw_sample_ct, nullptr);
          if ((rc == LDP_ERR_UNPHASED) && (bad_q != UINT32_MAX)) {
            die_unphased(inc[mk[bad_q]]);  // (chunks and launches run in variant order: the first one to fail holds the lowest variant)
          }
          if (rc) {
            die((rc == LDP_ERR_INVALID) ? 6 : 16, "\nError: %s: %s\n", gpath.c_str(), ldp_last_error(eng[r]));
          }
        }
        t_load_calls += now_s() - tl0;
        continue;
      }
      if (direct) {
        src = direct + static_cast<uint64_t>(raw0) * rec_bytes;
      } else {
        const double tw0 = now_s();
        decoder.join();
        t_wait_decode += now_s() - tw0;
        if (decode_rc == LDP_ERR_UNPHASED) {
          pending_unphased = unphased_at;  // reported below, unless a multiallelic variant before it is unphased too
          break;
        }
        if (decode_rc) {
          die(6, "\nError: %s: %s\n", gpath.c_str(), ldp_pgen_last_error(pg));
        }
        src = decoded[k & 1];
        start_decode(k + 1);
      }
      if ((!all_founders) && !device_subset) {
        // gather the founder columns (CopyNyparrNonemptySubset, pgenlib_misc.cc:32,185)
        // (+ CopyBitarrSubset of phaseinfo under --indep-pairphase, plink2_ld.cc:2075), all host threads
        gather.resize(static_cast<size_t>(run) * out_rec);
        if (ldp_subset_samples(src, direct ? rec_bytes : in_rec, run, raw_sample_ct, founder_mask.data(), gather.data(), out_rec, A.pairphase ? 1 : 0, 0)) {
          die(16, "\nError: founder subsetting failed.\n");
        }
        src = gather.data();
        stride = out_rec;
      }
      const double tl0 = now_s();
      for (int r = 0; r < world; ++r) {
        if (load_rows(eng[r], runs[k], src, stride)) {
          die(16, "Error: %s\n", ldp_last_error(eng[r]));
        }
      }
      t_load_calls += now_s() - tl0;
    }
    if (A.timing && !direct) {
      logprintf("\n[timing] variable-width records: %zu chunks, waited %.3f s for the decoder, %.3f s inside ldp_load_genotypes\n", runs.size(), t_wait_decode,
                t_load_calls);
    }
  }

  // rows that need host treatment overwrite their bulk-loaded versions: variants with more than one ALT
  // allele (collapsed major-vs-rest) and MT variants (hets -> missing, plink2_ld.cc:1362-1364)
  void patch_host_built_rows() {
    uint32_t multi_ct = 0, mt_ct = 0, multi_device = 0;
    // (--indep-pairphase: a multiallelic row is 2 haplotypes per founder as plain 2-bit codes on the 2N-haplotype engine)
    const uint64_t host_rec = A.pairphase ? ((2ull * founder_ct + 3) / 4) : out_rec;
    const uint64_t raw_phase_bytes = (static_cast<uint64_t>(raw_sample_ct) + 7) / 8;
    std::vector<uint8_t> lo(raw_sample_ct), hi(raw_sample_ct), inv_row(host_rec), raw_row(rec_bytes + 8), phase_buf(2 * raw_phase_bytes);
    uint32_t multi_unphased = UINT32_MAX;
    SexPlan mt_plan;
    mt_plan.part1 = founder_idx;
    // A multiallelic variant whose REF allele is the major one needs nothing: the main track already counts REF
    // copies (0/1/2 non-REF alleles = 0/1/2 non-major ones), and GetMajIdxMulti's first test (plink2_common.cc:1042,
    // freq[REF] >= 0.5 with freq = count * (1 / total), plink2_filter.cc:2137-2147) is the biallelic rule the
    // conversion kernel applied to the bulk-loaded row.  Its genotype counts say which variants those are.
    std::vector<uint8_t> ref_is_major;
    uint32_t multi_skipped = 0;
    if ((!A.pairphase) && !device_multi) {
      bool any_multi = false;
      for (uint32_t qq = 0; (qq < m_ct) && !any_multi; ++qq) {
        any_multi = (V.alt_ct[inc[mk[qq]]] > 1) && (vcls[mk[qq]] != 5);
      }
      if (any_multi) {
        ref_is_major.assign(m_ct, 0);
        std::vector<ldp_variant_rec> recs(m_ct);
        for (int r = 0; r < world; ++r) {  // (a variant's counts are zero on the engines that do not own it)
          must(eng[r], ldp_get_variant_recs(eng[r], 0, m_ct, recs.data()));
          for (uint32_t qq = 0; qq < m_ct; ++qq) {
            const uint64_t ref_ct = 2ull * recs[qq].n_homref + recs[qq].n_het;
            const uint64_t tot = 2ull * (static_cast<uint64_t>(recs[qq].n_homref) + recs[qq].n_het + recs[qq].n_homalt);
            if (tot && (static_cast<double>(ref_ct) * (1.0 / static_cast<double>(tot)) >= 0.5)) {
              ref_is_major[qq] = 1;
            }
          }
        }
      }
    }
    for (uint32_t qq = 0; qq < m_ct; ++qq) {
      const uint32_t raw_v = inc[mk[qq]];
      const uint32_t alts = V.alt_ct[raw_v];
      const bool is_mt = (vcls[mk[qq]] == 5);
      if (alts < 2 && !is_mt) {
        continue;
      }
      if (device_multi && !is_mt) {
        ++multi_device;  // (collapsed by ldp_load_pgen_records)
        continue;
      }
      if ((!is_mt) && (!ref_is_major.empty()) && ref_is_major[qq]) {
        ++multi_skipped;
        continue;
      }
      double mf = 0.0;
      if (is_mt && (alts >= 2)) {
        multiallelic_sex_row(pg, raw_v, alts, mt_plan, &lo, &hi, inv_row.data(), out_rec, &mf);
        ++mt_ct;
      } else if (is_mt) {
        fetch_raw_row(pg, storage_mode, raw_v, raw_sample_ct, rec_bytes, raw_row.data());
        build_sex_row(mt_plan, raw_row.data(), inv_row.data(), out_rec, &mf);
        ++mt_ct;
      } else {
        if (storage_mode == 0x01) {
          die(6, "\nError: multiallelic variant in a .bim/.bed fileset.\n");
        }
        if (A.pairphase) {
          bool unphased = false;
          multiallelic_inverse_row(pg, raw_v, alts, founder_idx, &lo, &hi, inv_row.data(), host_rec, &mf, phase_buf.data(), raw_phase_bytes, &unphased);
          if (unphased) {
            multi_unphased = std::min(multi_unphased, raw_v);
          }
        } else {
          multiallelic_inverse_row(pg, raw_v, alts, founder_idx, &lo, &hi, inv_row.data(), out_rec, &mf);
        }
        ++multi_ct;
      }
      for (int r = 0; r < world; ++r) {
        must(eng[r], ldp_load_genotypes(eng[r], qq, 1, inv_row.data(), host_rec, LDP_MEM_HOST, LDP_GENO_INVERSE));
        must(eng[r], ldp_set_maj_freqs(eng[r], qq, 1, &mf));
      }
    }
    if (std::min(multi_unphased, pending_unphased) != UINT32_MAX) {
      die_unphased(std::min(multi_unphased, pending_unphased));
    }
    if ((multi_ct || mt_ct || multi_skipped || multi_device) && A.timing) {
      logprintf("\n[timing] host-built rows: %u multiallelic (%u more have REF as the major allele: main track as loaded; %u collapsed on the device), %u MT\n",
                multi_ct, multi_skipped, multi_device, mt_ct);
    }
  }

  // Variants whose records carry dosages: the major allele's frequency comes from the founders' dosage sums (a sample's
  // dosage where it has one, its hardcall otherwise: ldp_pgen_dosage_sums), in ComputeAlleleFreqs' arithmetic
  // (plink2_filter.cc:2137-2147: ref * (1 / (ref + alt)); the factor 2 of the diploid case cancels exactly) with
  // GetMajIdx's rule (REF unless its frequency is below 0.5).  The rows themselves stay the hardcalls.
  void set_dosage_frequencies() {
    if (S.has_dosage) {
      const double t_dos0 = now_s();
      std::vector<uint32_t> todo;
      for (uint32_t qq = 0; qq < m_ct; ++qq) {
        const uint32_t raw_v = inc[mk[qq]];
        if (!ldp_pgen_variant_has_dosage(pg, raw_v)) {
          continue;
        }
        if ((V.alt_ct[raw_v] > 1) || (vcls[mk[qq]] == 5)) {
          die(63, "\nError: variant '%s' has dosages and %s, which plink2-hip does not read yet.\n", V.id[raw_v].c_str(),
              (vcls[mk[qq]] == 5) ? "lies on chrM" : "several ALT alleles");
        }
        todo.push_back(qq);
      }
      std::vector<double> mfs(todo.size(), 0.0);
      size_t from_device = 0, from_host = 0;
      {
        std::vector<uint32_t> raw_todo(todo.size());
        for (size_t q = 0; q < todo.size(); ++q) {
          raw_todo[q] = inc[mk[todo[q]]];
        }
        // The engine that loaded a variant's record summed its dosage track where the bytes landed (ldp_load_pgen_records ->
        // ldp_get_dosage_sums; under --gpus N every run lies in the engine that owns it).  What is left -- --debug-host-decode,
        // --indep-pairphase rows, rows the host built -- takes the host pass over the file.
        std::vector<uint32_t> host_todo;
        if (!todo.empty()) {
          const uint32_t q_lo = todo.front(), q_n = todo.back() - todo.front() + 1;
          std::vector<uint64_t> ref_dd(q_n), alt_dd(q_n);
          std::vector<uint8_t> has(q_n), any(q_n, 0);
          std::vector<std::pair<uint64_t, uint64_t>> got(q_n);
          for (int r = 0; (r < world) && !g_dbg.host_decode; ++r) {
            must(eng[r], ldp_get_dosage_sums(eng[r], q_lo, q_n, ref_dd.data(), alt_dd.data(), has.data()));
            for (uint32_t k = 0; k < q_n; ++k) {
              if (has[k] && !any[k]) {
                any[k] = 1;
                got[k] = {ref_dd[k], alt_dd[k]};
              }
            }
          }
          for (size_t q = 0; q < todo.size(); ++q) {
            if (S.dosage_sums.count(raw_todo[q])) {
              continue;  // (the host's filter pass before the load has them)
            }
            const uint32_t k = todo[q] - q_lo;
            if (any[k]) {
              S.dosage_sums[raw_todo[q]] = got[k];
              ++from_device;
            } else {
              host_todo.push_back(raw_todo[q]);
            }
          }
        }
        from_host = host_todo.size();
        S.need_dosage_sums(host_todo);
        for (size_t q = 0; q < todo.size(); ++q) {
          const std::pair<uint64_t, uint64_t>& dd = S.dosage_sums[raw_todo[q]];
          const uint64_t tot = dd.first + dd.second;
          const double ref_freq = tot ? (static_cast<double>(static_cast<int64_t>(dd.first)) * (1.0 / static_cast<double>(static_cast<int64_t>(tot)))) : 0.5;
          mfs[q] = (ref_freq < 0.5) ? (1.0 - ref_freq) : ref_freq;
        }
      }
      // one call per run of consecutive variants per engine
      for (size_t q = 0; q < todo.size();) {
        size_t run = 1;
        while ((q + run < todo.size()) && (todo[q + run] == todo[q] + run)) {
          ++run;
        }
        for (int r = 0; r < world; ++r) {
          must(eng[r], ldp_set_maj_freqs(eng[r], todo[q], static_cast<uint32_t>(run), &mfs[q]));
        }
        q += run;
      }
      if (A.timing) {
        // (what lies between the end of the load and the first pair launch: this pass, and the rows the host builds before it)
        logprintf("\n[timing] allele frequencies of %zu variants from their dosages: %zu summed on the device by the load, %zu by the host pass over the file, %.3f s "
                  "(rows loaded in %.3f s; %.3f s from the end of the load to the end of this pass)\n",
                  todo.size(), from_device, from_host, now_s() - t_dos0, t_rows1 - t_rows0, now_s() - t_rows1);
      }
    }
  }

  // --mind from the resident image (Session::mind_device): every row the table filters leave is loaded -- chromosome 0 included, under the all-pairs
  // plan --, ldp_sample_missing_counts() reads the image once in the sample direction, and MindFilter's rule (mind_decide, the one the host pass
  // uses) decides.  Nobody goes: false, and the run goes on with the image it has.  Somebody goes: the image's columns cannot be dropped in place,
  // so the engine is destroyed and true tells run() to hand the decision back to main(), which starts over with those samples excluded.
  bool mind_on_device() {
    if (m_ct != S.mind_variant_ct) {
      die(16, "\nError: internal: --mind counted %u variants on the host's list and %u rows are loaded.\n", S.mind_variant_ct, m_ct);
    }
    std::vector<uint32_t> by_column(std::max<uint32_t>(founder_ct, 1), 0);
    must(eng[0], ldp_sample_missing_counts(eng[0], 0, m_ct, by_column.data()));
    std::vector<uint32_t> missing_cts;
    to_file_order(by_column, &missing_cts);
    std::vector<uint8_t> removed_samples;
    const uint32_t removed_ct = mind_decide(S, missing_cts, &removed_samples);
    if (A.timing) {
      double ms = 0.0;
      uint64_t bytes = 0;
      (void)ldp_debug_get_sample_missing_stats(eng[0], &ms, &bytes);
      logprintf("[timing] sample filter (--mind): from the resident image (%u rows, %.3f ms = %.0f GB/s; %u sample%s removed%s)\n", m_ct, ms,
                gb_per_s(static_cast<double>(bytes), ms * 1e-3), removed_ct, (removed_ct == 1) ? "" : "s", removed_ct ? ", reloading" : "");
    }
    if (!removed_ct) {
      return false;
    }
    mind_apply(S, removed_samples);  // (exit 13 when nobody is left)
    ldp_destroy(eng[0]);
    eng.clear();
    S.file_to_hbm_done();
    S.mind_removed = removed_samples;
    S.restart = true;
    return true;
  }

  // --missing / --freq / --geno-counts from the same load (Session::report_device): the records of the count pass hold every listed row's
  // non-missing count and three genotype counts, the image its per-sample missing calls (ldp_sample_missing_counts), and a row with several
  // ALT alleles the allele counts its major allele was chosen from (ldp_get_allele_counts; a row the host builds has none: the reader's
  // allele pairs are counted instead).  Every kept sample is a founder here, so one set of counts serves all three reports.  Before
  // ldp_restrict_variants(): the reports list what the table filters leave, chromosome 0 included.
  void reports_on_device() {
    const double t0 = now_s();
    if ((m_ct != S.report_variants.size()) || (m_ct != variant_ct)) {
      die(16, "\nError: internal: the reports list %zu variants and %u rows are loaded.\n", S.report_variants.size(), m_ct);
    }
    const std::vector<ldp_variant_rec> recs = recs_of(eng[0]);
    ReportCounts C;
    C.kept_sample_ct = founder_ct;
    C.variants.resize(m_ct);
    C.missing.resize(m_ct);
    C.f_ref2.resize(m_ct);
    C.f_het.resize(m_ct);
    C.f_alt2.resize(m_ct);
    std::vector<uint32_t> offsets(static_cast<size_t>(m_ct) + 1, 0);
    for (uint32_t q = 0; q < m_ct; ++q) {
      const uint32_t raw_v = inc[mk[q]];
      if (raw_v != S.report_variants[q]) {
        die(16, "\nError: internal: row %u holds variant %u, the reports list %u there.\n", q, raw_v, S.report_variants[q]);
      }
      C.variants[q] = raw_v;
      C.missing[q] = founder_ct - recs[q].nm_ct;
      C.f_ref2[q] = recs[q].n_homref;
      C.f_het[q] = recs[q].n_het;
      C.f_alt2[q] = recs[q].n_homalt;
      offsets[q + 1] = offsets[q] + ((A.rep_freq && (V.alt_ct[raw_v] > 1)) ? (static_cast<uint32_t>(V.alt_ct[raw_v]) + 1) : 0u);
    }
    size_t multi_device = 0, multi_host = 0;
    if (offsets[m_ct]) {
      std::vector<uint32_t> counts(offsets[m_ct]);
      std::vector<uint8_t> has(m_ct), lo, hi;
      must(eng[0], ldp_get_allele_counts(eng[0], 0, m_ct, offsets.data(), counts.data(), has.data()));
      for (uint32_t q = 0; q < m_ct; ++q) {
        if (offsets[q + 1] == offsets[q]) {
          continue;
        }
        std::vector<uint32_t>& dst = C.allele_cts[q];
        if (has[q]) {
          dst.assign(counts.begin() + offsets[q], counts.begin() + offsets[q + 1]);
          ++multi_device;
        } else {
          reports_count_alleles_host(S, C.variants[q], &lo, &hi, &dst);
          ++multi_host;
        }
      }
    }
    C.sample_missing.assign(raw_sample_ct, 0);
    if (A.rep_smiss()) {
      std::vector<uint32_t> by_column(std::max<uint32_t>(founder_ct, 1), 0);
      must(eng[0], ldp_sample_missing_counts(eng[0], 0, m_ct, by_column.data()));
      to_file_order(by_column, &C.sample_missing);
    }
    const double t1 = now_s();
    write_reports(S, C);
    if (A.timing) {
      logprintf("[timing] reports: from the device's count pass (%u rows; records%s %.3f s, writing %.3f s; allele counts of %zu multiallelic rows from the device, %zu from the reader)\n",
                m_ct, A.rep_smiss() ? " and the per-sample read of the image" : "", t1 - t0, now_s() - t1, multi_device, multi_host);
    }
  }

  // --het from the resident image (Session::het_device), after the filters and on the restricted engine: the records of the count pass give
  // every row's genotype counts, hence its expected heterozygosity (het_expected) and the integer weight it enters the sums with (HetPlan);
  // one ldp_sample_het_counts() call reads the image in the sample direction -- het calls, missing calls and the summed weights of the missing
  // calls per column --, and the writer the host's pass uses does the rest.  One engine, autosomes only, no multiallelic variant, every kept
  // sample a founder: row q is variant q of the list, column f founder f of the file.
  void het_on_device() {
    const double t0 = now_s();
    if (m_ct != variant_ct) {
      die(16, "\nError: internal: --het lists %u variants and %u rows are loaded.\n", variant_ct, m_ct);
    }
    het_preamble(S, m_ct, 0);
    const std::vector<ldp_variant_rec> recs = recs_of(eng[0]);
    std::vector<double> ehet(m_ct, 0.0);
    std::vector<uint8_t> ok(m_ct, 0);
    for (uint32_t q = 0; q < m_ct; ++q) {
      const uint32_t cts[2] = {2 * recs[q].n_homref + recs[q].n_het, 2 * recs[q].n_homalt + recs[q].n_het};
      ok[q] = het_expected(cts, 2, A.het_small_sample, &ehet[q]) ? 1 : 0;
      if (ok[q] && (!direct_rows) && !recs[q].nm_ct) {
        ok[q] = 0;  // (het_all_missing_skipped, p2h_cli.h: the kept samples are the founders here)
      }
    }
    HetPlan plan;
    plan.build(ehet, ok);
    const uint32_t cols = std::max<uint32_t>(founder_ct, 1);
    std::vector<uint32_t> het_col(cols, 0), mis_col(cols, 0);
    std::vector<uint64_t> mw_col(cols, 0);
    double ms = 0.0;
    uint64_t bytes = 0;
    // (--timing: the same pass through its measurement hook, which also returns the kernel's time and the bytes it read)
    must(eng[0], A.timing ? ldp_debug_sample_het_counts(eng[0], 0, m_ct, plan.include.data(), plan.weight.data(), het_col.data(), mis_col.data(), mw_col.data(), 0, &ms, &bytes)
                          : ldp_sample_het_counts(eng[0], 0, m_ct, plan.include.data(), plan.weight.data(), het_col.data(), mis_col.data(), mw_col.data()));
    HetSums sums;
    to_file_order(het_col, &sums.het_ct);
    to_file_order(mis_col, &sums.missing_ct);
    to_file_order(mw_col, &sums.missing_weight);
    const double t1 = now_s();
    het_write(S, plan, sums);
    if (A.timing) {
      logprintf("[timing] --het: from the resident image (%u rows, %u of them kept; kernel %.3f ms = %.0f GB/s; records, plan and the call %.3f s, writing %.3f s)\n", m_ct, plan.kept, ms,
                gb_per_s(static_cast<double>(bytes), ms * 1e-3), t1 - t0, now_s() - t1);
    }
  }
  void het_stage() {
    if (S.het_device) {
      het_on_device();
    } else {
      het_host_pass(S);
    }
  }

  // --make-king-table from the resident image (Session::king_device; the conditions of het_on_device: row q is variant q of the list, column f
  // founder f of the file = kept sample f).  Row blocks of samples against every earlier sample, sized so that a block holds at most 2^24 pairs
  // (the library keeps 20 bytes per pair of the block on the device): the dense form without --king-table-filter, the hit form with it -- the
  // device drops the pairs below the threshold, the writer forms the doubles it prints from the returned integers again -- and either way the
  // lines leave in the table's order, row ascending, column ascending.
  void king_on_device() {
    const double t0 = now_s();
    if (m_ct != variant_ct) {
      die(16, "\nError: internal: --make-king-table lists %u variants and %u rows are loaded.\n", variant_ct, m_ct);
    }
    king_preamble(S, founder_ct, m_ct, 0);
    KingWriter w(S);
    const uint64_t kBlockPairs = 1ull << 24;
    std::vector<ldp_king_counts_t> dense;
    std::vector<ldp_king_hit> hits;
    double ms_total = 0.0, call_s = 0.0;
    uint64_t pair_variants = 0;
    uint32_t blocks = 0;
    for (uint32_t r0 = 1; r0 < founder_ct;) {
      // rows [r0, r1) against columns [0, r1 - 1)
      uint32_t rows = static_cast<uint32_t>(std::min<uint64_t>(4096, std::max<uint64_t>(32, kBlockPairs / (static_cast<uint64_t>(r0) + 32))));
      rows = std::min(rows, founder_ct - r0);
      while ((rows > 32) && (static_cast<uint64_t>(rows) * (r0 + rows - 1) > kBlockPairs)) {
        rows = std::max(32u, rows / 2);
      }
      const uint32_t r1 = r0 + rows, cols = r1 - 1;
      const uint64_t block_pairs = (static_cast<uint64_t>(r1) * (r1 - 1) - static_cast<uint64_t>(r0) * (r0 - 1)) / 2;
      const double tc = now_s();
      if (A.king_filter_given) {
        if (hits.empty()) {
          hits.resize(1u << 20);
        }
        uint64_t found = 0;
        for (int attempt = 0; attempt < 2; ++attempt) {
          must(eng[0], ldp_king_block_hits(eng[0], 0, m_ct, nullptr, r0, rows, 0, cols, A.king_filter, hits.data(), hits.size(), &found));
          if (found <= hits.size()) {
            break;
          }
          hits.resize(found);  // (more pairs pass than the list held: once more with room for all of them)
        }
        call_s += now_s() - tc;
        std::sort(hits.begin(), hits.begin() + found, [](const ldp_king_hit& a, const ldp_king_hit& b) { return (a.row != b.row) ? (a.row < b.row) : (a.col < b.col); });
        for (uint64_t k = 0; k < found; ++k) {
          w.pair(hits[k].row, hits[k].col, hits[k].c);
        }
        w.add_filtered(block_pairs - found);
        pair_variants += block_pairs * m_ct;
      } else {
        dense.resize(static_cast<size_t>(rows) * cols);
        double ms = 0.0;
        uint64_t pv = 0;
        must(eng[0], ldp_debug_king_counts_block(eng[0], 0, m_ct, nullptr, r0, rows, 0, cols, dense.data(), cols, 0, &ms, &pv));
        call_s += now_s() - tc;
        ms_total += ms;
        pair_variants += pv;
        for (uint32_t i = r0; i < r1; ++i) {
          const ldp_king_counts_t* row = dense.data() + static_cast<size_t>(i - r0) * cols;
          for (uint32_t j = 0; j < i; ++j) {
            w.pair(i, j, row[j]);
          }
        }
      }
      ++blocks;
      r0 = r1;
    }
    w.finish(m_ct);
    if (A.timing) {
      const double total = now_s() - t0;
      if (A.king_filter_given) {
        logprintf("[timing] --make-king-table: from the resident image (%u samples, %u rows, %u blocks, hit form; the calls %.3f s = %.3g pair-variants/s; sorting and writing %.3f s)\n",
                  founder_ct, m_ct, blocks, call_s, (call_s > 0.0) ? (static_cast<double>(pair_variants) / call_s) : 0.0, total - call_s);
      } else {
        logprintf("[timing] --make-king-table: from the resident image (%u samples, %u rows, %u blocks, dense form; kernels %.3f ms = %.3g pair-variants/s; the calls %.3f s, writing %.3f s)\n",
                  founder_ct, m_ct, blocks, ms_total, (ms_total > 0.0) ? (static_cast<double>(pair_variants) / (ms_total * 1e-3)) : 0.0, call_s, total - call_s);
      }
    }
  }
  void king_stage() {
    if (S.king_device) {
      king_on_device();
    } else {
      king_host_pass(S);
    }
  }

  // --geno / --maf / --max-maf / --mac / --max-mac from the records the load's own count pass left on the device (nm_ct and the three
  // genotype counts of every row, over the founders = the kept samples: device_filter_refusal): the arithmetic of the host's pass
  // (CountFilters), then the engine drops the variants that go and plans over the rest (ldp_restrict_variants), and the session's variant
  // tables follow.  One engine, autosomes only, no multiallelic variant: mk is every variant.
  void filter_on_device() {
    const double t0 = now_s();
    const std::vector<ldp_variant_rec> recs = recs_of(eng[0]);
    CountFilters F(A, S.kept_sample_ct);
    // --hwe / --hardy: ln p of every row from the same records, where they lie (hwe_kernel through ldp_hwe_ln_pvals: no copy of the records,
    // no host thread); one call serves both where their `midp` settings agree.  (--timing: the call through its measurement hook)
    std::vector<double> ln_hwe, ln_hardy;
    if (A.hwe || A.hardy) {
      const int midp_first = A.hwe ? (A.hwe_midp ? 1 : 0) : (A.hardy_midp ? 1 : 0);
      std::vector<uint8_t> flags(std::max<uint32_t>(m_ct, 1), 0);
      auto pvals = [&](int midp, std::vector<double>* out) {
        out->assign(std::max<uint32_t>(m_ct, 1), 0.0);
        double ms = 0.0;
        must(eng[0], ldp_debug_hwe_ln_pvals(eng[0], 0, m_ct, midp, out->data(), flags.data(), &ms));
        hwe_ms_kernel += ms;
        hwe_pvals += m_ct;
        for (uint32_t q = 0; q < m_ct; ++q) {
          hwe_ties += flags[q] & 1;
        }
      };
      pvals(midp_first, &ln_hwe);
      if (A.hwe && A.hardy && (A.hwe_midp != A.hardy_midp)) {
        pvals(A.hardy_midp ? 1 : 0, &ln_hardy);
      }
      if (A.timing) {  // (here, not with the other filter timings: --hwe's strictness error ends the run before those)
        logprintf("[timing] --hwe / --hardy: from the device's records (%llu p-values, hwe_kernel %.3f ms; %u with a tolerance tie)\n", static_cast<unsigned long long>(hwe_pvals), hwe_ms_kernel,
                  hwe_ties);
      }
    }
    HardyCounts H;
    std::vector<uint64_t> keep((static_cast<size_t>(m_ct) + 63) / 64 + 1, 0);
    uint32_t kept = 0, chr0_left = 0;
    for (uint32_t q = 0; q < m_ct; ++q) {
      const ldp_variant_rec& r = recs[q];
      if (A.hardy && !F.fails_geno(founder_ct - r.nm_ct)) {
        H.add(S.inc[q], r.n_homref, r.n_het, r.n_homalt, ln_hardy.empty() ? ln_hwe[q] : ln_hardy[q]);
      }
      if (!F.drops(founder_ct - r.nm_ct, r.n_homref, r.n_het, r.n_homalt, nullptr, ln_hwe.empty() ? nullptr : &ln_hwe[q])) {
        if ((q < S.inc_chr0.size()) && S.inc_chr0[q]) {
          ++chr0_left;  // (never pruned, never listed: LdPrune strips chromosome 0, plink2_ld.cc:2542)
          continue;
        }
        keep[q >> 6] |= 1ull << (q & 63);
        // (mk[q] == q here: the tables are compacted in place)
        S.inc[kept] = S.inc[q];
        S.chr_idx[kept] = S.chr_idx[q];
        S.bps[kept] = S.bps[q];
        S.vcls[kept] = S.vcls[q];
        ++kept;
      }
    }
    F.log_counts([&]() {
      if (A.hardy) {
        write_hardy(S, H);
      }
    });
    if ((!kept) && !chr0_left) {  // plink2.cc:2484-2487 (kPglRetDegenerateData)
      filter_s = now_s() - t0;
      report_filter_timing();
      die(13, "Error: No variants remaining after main filters.\n");
    }
    if (chr0_left) {
      logprintf("--indep-pairwise: Ignoring %u chromosome 0 variant%s.\n", chr0_left, chr0_left == 1 ? "" : "s");
    }
    S.inc_chr0.clear();
    S.inc.resize(kept);
    S.chr_idx.resize(kept);
    S.bps.resize(kept);
    S.vcls.resize(kept);
    S.mk.resize(kept);
    S.m_chr = S.chr_idx;
    S.m_bps = S.bps;
    S.variant_ct = S.m_ct = variant_ct = m_ct = kept;
    for (uint32_t k = 1; A.window_is_bp && (k < kept); ++k) {
      if ((chr_idx[k] == chr_idx[k - 1]) && (bps[k] < bps[k - 1])) {  // plink2.cc:2926-2929
        die(6, "Error: When the window size is in kb units, LD-based pruning requires a sorted\n.pvar/.bim.  Retry this command after using --make-pgen/--make-bed +\n--sort-vars to sort your data.\n");
      }
    }
    must(eng[0], ldp_restrict_variants(eng[0], keep.data(), kept, m_chr.data(), A.window_is_bp ? m_bps.data() : nullptr));
    ldp_get_subcontigs(eng[0], &subcontig_ct, nullptr, 0);
    (void)ldp_debug_get_compact_stats(eng[0], &filter_rows_compacted, nullptr, &filter_rows_bounced, &filter_ms_compact);
    removed.assign((static_cast<size_t>(variant_ct) + 63) / 64 + 1, 0);
    if (A.timing && kept) {
      // (the count pass that ran over the kept rows in place: fetching the records -- the run wants them anyway -- closes its event pair)
      ldp_variant_rec first;
      ldp_counters c;
      if ((ldp_get_variant_recs(eng[0], 0, 1, &first) == LDP_OK) && (ldp_get_counters(eng[0], &c) == LDP_OK)) {
        filter_ms_recount = c.ms_prepare;
      }
    }
    filter_s = now_s() - t0;
  }

  void report_filter_timing() {
    if ((!A.timing) || !S.count_filters) {  // (--mind alone takes this path too: no variant filter to report)
      return;
    }
    logprintf("[timing] variant filters: from the device's count pass (%llu rows compacted, %.3f ms; records, filter arithmetic and the new plan %.3f s in all)\n",
              static_cast<unsigned long long>(filter_rows_compacted), filter_ms_compact, filter_s);

    if ((founder_ct <= ldp_matrix_pipe_max_founders()) && (filter_ms_compact > 0.0) && (filter_ms_recount > 0.0)) {
      // image rows of ceil(founders / 512) x 128 bytes: the compaction reads and writes a moved row once, twice when its batch goes through the bounce
      // buffer (few rows dropped in front of it); the count pass reads the kept rows
      const double pitch = static_cast<double>((static_cast<uint64_t>(founder_ct) + 511) / 512 * 128);
      const double moved_gb = static_cast<double>(filter_rows_compacted) * pitch / 1e9, kept_gb = static_cast<double>(m_ct) * pitch / 1e9;
      const double traffic_gb = 2.0 * static_cast<double>(filter_rows_compacted + filter_rows_bounced) * pitch / 1e9;
      logprintf("[timing] compaction: %.3f GB of rows moved, %llu of %llu rows through the bounce buffer: %.3f GB of HBM traffic in %.3f ms = %.0f GB/s; the count pass over the kept rows in place: %.3f GB read in %.3f ms = %.0f GB/s\n",
                moved_gb, static_cast<unsigned long long>(filter_rows_bounced), static_cast<unsigned long long>(filter_rows_compacted), traffic_gb, filter_ms_compact,
                traffic_gb / (filter_ms_compact * 1e-3), kept_gb, filter_ms_recount, kept_gb / (filter_ms_recount * 1e-3));
    }
  }

  // every engine prunes its shard; several engines: their removed-bit segments meet (stitch, plink2_ld.cc:1418-1426)
  void run_diploid_engines() {
    t_load1 = now_s();
    const std::vector<uint64_t> pref_m = sub_preferred(mk);
    const size_t m_words = (static_cast<size_t>(m_ct) + 63) / 64 + 1;
    std::vector<std::vector<uint64_t>> part(world, std::vector<uint64_t>(m_words, 0));
    std::vector<int> rcs(world, 0);
    // several devices: every engine prunes its shard on a host thread of its own; the shards' results then meet in ONE RCCL
    // all-gather of their removed-bit segments (ldp_allgather_removed: the cross-device form of the stitch at
    // plink2_ld.cc:1418-1426).  Without RCCL -- or with engines that share a device -- the same segments are packed, copied
    // between the engines by the host and stitched by every rank (ldp_pack_removed_segment / ldp_stitch_removed_segments).
    std::vector<std::thread> th;
    for (int r = 0; r < world; ++r) {
      th.emplace_back([&, r]() {
        if (!pref_m.empty()) {
          ldp_set_preferred(eng[r], pref_m.data());
        }
        rcs[r] = ldp_run(eng[r], part[r].data());
      });
    }
    for (std::thread& t : th) {
      t.join();
    }
    th.clear();
    // (a rank whose run failed must not leave the others waiting in a collective: nobody enters it then)
    for (int r = 0; r < world; ++r) {
      must(eng[r], rcs[r]);
    }
    if (world == 1) {
      scatter(part[0], mk);
    } else {
      std::vector<void*> comms(world, nullptr);
      std::vector<std::vector<uint64_t>> full(world, std::vector<uint64_t>(m_words, 0));
      bool use_rccl = false;
      if (!alias_devices) {
        std::vector<int> devs(world);
        for (int r = 0; r < world; ++r) {
          devs[r] = r;
        }
        use_rccl = (ldp_comm_init_all(world, devs.data(), comms.data()) == 0);
      }
      if (use_rccl) {
        for (int r = 0; r < world; ++r) {
          th.emplace_back([&, r]() { rcs[r] = ldp_allgather_removed(eng[r], comms[r], part[r].data(), full[r].data()); });
        }
        for (std::thread& t : th) {
          t.join();
        }
        for (int r = 0; r < world; ++r) {
          must(eng[r], rcs[r]);  // (the failing rank aborted its communicator; the process ends here, nothing is destroyed twice)
        }
        for (int r = 0; r < world; ++r) {
          ldp_comm_destroy(comms[r]);
        }
      } else {
        uint64_t seg_words = 0;
        must(eng[0], ldp_shard_segment_words(eng[0], &seg_words));
        std::vector<uint64_t> segs(static_cast<size_t>(seg_words) * world, 0);
        for (int r = 0; r < world; ++r) {
          if (ldp_pack_removed_segment(eng[r], part[r].data(), segs.data() + static_cast<size_t>(r) * seg_words)) {
            die(16, "\nError: packing the removed bits of shard %d failed.\n", r);
          }
        }
        for (int r = 0; r < world; ++r) {
          if (ldp_stitch_removed_segments(eng[r], segs.data(), full[r].data())) {
            die(16, "\nError: stitching the removed bits on shard %d failed.\n", r);
          }
        }
      }
      for (int r = 1; r < world; ++r) {  // every rank holds the same global bitmap
        if (memcmp(full[r].data(), full[0].data(), ((static_cast<size_t>(m_ct) + 63) / 64) * sizeof(uint64_t)) != 0) {
          die(16, "\nError: the shards disagree about the stitched prune bitmap (rank %d).\n", r);
        }
      }
      scatter(full[0], mk);
      if (A.timing) {
        logprintf("\n[timing] %d engines on %d device%s, exchange: %s\n", world, std::min(world, n_devices), (std::min(world, n_devices) == 1) ? "" : "s",
                  use_rccl ? "RCCL all-gather" : "host transport");
      }
    }
    t_run1 = now_s();
  }

  void report_load_and_run() {
    ldp_counters c;
    ldp_get_counters(eng[0], &c);
    logprintf("\n[timing] setup+parse %.3f s | genotype load (file -> HBM bit-planes) %.3f s | run %.3f s (pair kernel %.1f ms, replay %.1f ms; %llu candidate pairs) | buffer release %.3f s\n",
              t_load0 - t_begin, t_load1 - t_load0, (t_run1 ? t_run1 : now_s()) - t_load1, c.ms_pair_kernel, c.ms_replay, static_cast<unsigned long long>(c.candidate_pairs), t_run1 ? now_s() - t_run1 : 0.0);
    // which pair kernels the device-side route gave engine 0's launches (ldp_counters; the dispatch of plink2_ld.cc:699-723, per launch)
    logprintf("[timing] pair launches by route: complete data %u | a few missing calls %u (%u on the 8 x 8 tiles) | missing calls %u (%u on quarter tiles) | %u tiles planned, %llu pairs recounted exactly\n",
              c.route_complete_launches, c.route_sparse_launches, c.sparse_tile_launches, c.route_general_launches, c.four_tile_launches, c.wide_tiles,
              static_cast<unsigned long long>(c.sparse_exact_pairs));
    // ... and, where the launches gave every 8 x 8 tile the class of its own rows (ldp_get_tile_routes), the tiles by the kernel they ran on
    ldp_tile_routes tr;
    if ((ldp_get_tile_routes(eng[0], &tr) == LDP_OK) && (tr.tiles_complete | tr.tiles_sparse | tr.tiles_general)) {
      logprintf("[timing] tiles by their own rows: complete data %llu | a few missing calls %llu | missing calls %llu (quarter tiles) | %llu corner products handed over\n",
                static_cast<unsigned long long>(tr.tiles_complete), static_cast<unsigned long long>(tr.tiles_sparse), static_cast<unsigned long long>(tr.tiles_general),
                static_cast<unsigned long long>(tr.corner_products));
    }
  }

  // ---- chrX, chrY: their own sample sets, rows built on the host, one engine each on device 0
  // (--indep-pairphase: MT too, one haplotype per founder with hets missing -- HapsplitHaploid, plink2_ld.cc:2051)
  void run_sex_chromosomes() {
    for (int which = 0; which < 3; ++which) {
      const std::vector<uint32_t>& ks = (which == 0) ? xk : ((which == 1) ? yk : tk);
      if (ks.empty()) {
        continue;
      }
      static const char* const kSexName[3] = {"X", "Y", "MT"};
      SexPlan sp;
      for (uint32_t sidx : founder_idx) {
        if (which == 0) {
          (sex[sidx] == 1 ? sp.part1 : sp.part2).push_back(sidx);  // males | non-males (female + unknown)
        } else if ((which == 2) || (sex[sidx] != 2)) {
          sp.part1.push_back(sidx);                                  // non-females (chrY) / every founder (MT)
        }
      }
      sp.x_freq = (which == 0);
      const bool x_phased = A.pairphase && (which == 0) && !sp.part2.empty();
      std::vector<uint8_t> nonmale_mask;
      if (x_phased) {  // (sp.part2: the founders that are not male)
        nonmale_mask = sample_mask(raw_sample_ct, [&](uint32_t s) { return is_founder[s] && (sex[s] != 1); });
      }
      const uint32_t fct = sp.out_ct();
      if (fct < 2) {
        die(63, "\nError: fewer than two usable founders on chr%s; not supported by plink2-hip.\n", kSexName[which]);
      }
      ldp_params SP = P;
      SP.founder_ct = fct;
      SP.device = 0;
      ldp_engine* se = nullptr;
      std::vector<uint32_t> s_chr(ks.size()), s_bps(ks.size());
      for (size_t w = 0; w < ks.size(); ++w) {
        s_chr[w] = chr_idx[ks[w]];
        s_bps[w] = bps[ks[w]];
      }
      if (ldp_create(&SP, &se) || ldp_set_variants(se, static_cast<uint32_t>(ks.size()), s_chr.data(), A.window_is_bp ? s_bps.data() : nullptr)) {
        die(16, "\nError: chr%s engine setup failed.\n", kSexName[which]);
      }
      const uint64_t s_rec = (static_cast<uint64_t>(fct) + 3) / 4;
      const uint32_t chunk = std::max<uint32_t>(1, static_cast<uint32_t>((256ull << 20) / std::max<uint64_t>(s_rec, 1)));
      std::vector<uint8_t> rows;
      std::vector<double> mfs;
      std::atomic<uint32_t> x_unphased(UINT32_MAX);
      if (!x_phased) {
        // The rows are built on the device (ldp_set_sample_map): the file's rows go up as they are, in runs of variants
        // that are consecutive in the file, and a conversion-time gather picks the founders -- the haploid ones first, with
        // their het calls made missing, then (chrX) the others twice.  The host used to do this per sample and variant.
        std::vector<uint32_t> src_sample;
        std::vector<uint8_t> het_missing;
        src_sample.reserve(fct);
        het_missing.reserve(fct);
        for (uint32_t sidx : sp.part1) {
          src_sample.push_back(sidx);
          het_missing.push_back(1);
        }
        for (int rep = 0; rep < 2; ++rep) {
          for (uint32_t sidx : sp.part2) {
            src_sample.push_back(sidx);
            het_missing.push_back(0);
          }
        }
        must(se, ldp_set_sample_map(se, raw_sample_ct, src_sample.data(), het_missing.data()));
        const uint32_t max_run = std::max<uint32_t>(1, static_cast<uint32_t>((256ull << 20) / std::max<uint64_t>(rec_bytes, 1)));
        std::vector<uint8_t> decoded;
        for (uint32_t w0 = 0; w0 < ks.size();) {
          const uint32_t raw0 = inc[ks[w0]];
          uint32_t run = 1;
          while ((w0 + run < ks.size()) && (inc[ks[w0 + run]] == raw0 + run) && (run < max_run)) {
            ++run;
          }
          const uint8_t* rows_at = nullptr;
          if (direct_rows) {
            rows_at = direct_rows + static_cast<uint64_t>(raw0) * rec_bytes;
          } else {
            decoded.resize(static_cast<size_t>(run) * rec_bytes);
            if (ldp_pgen_read(pg, raw0, run, decoded.data(), rec_bytes, 0)) {
              die(6, "\nError: %s: %s\n", gpath.c_str(), ldp_pgen_last_error(pg));
            }
            rows_at = decoded.data();
          }
          must(se, ldp_load_genotypes(se, w0, run, rows_at, rec_bytes, LDP_MEM_HOST, encoding | LDP_GENO_MAPPED));
          w0 += run;
        }
        // variants with several ALT alleles: their rows (collapsed on the major allele of the chromosome's own allele-frequency rule) are
        // built here and replace the mapped main tracks
        std::vector<uint8_t> lo_a, hi_a, m_row;
        for (uint32_t w = 0; w < ks.size(); ++w) {
          const uint32_t raw_v = inc[ks[w]];
          if (V.alt_ct[raw_v] < 2) {
            continue;
          }
          if (lo_a.empty()) {
            lo_a.resize(raw_sample_ct);
            hi_a.resize(raw_sample_ct);
            m_row.resize(s_rec);
          }
          double mf = 0.0;
          multiallelic_sex_row(pg, raw_v, V.alt_ct[raw_v], sp, &lo_a, &hi_a, m_row.data(), s_rec, &mf);
          must(se, ldp_load_genotypes(se, w, 1, m_row.data(), s_rec, LDP_MEM_HOST, LDP_GENO_INVERSE));
          must(se, ldp_set_maj_freqs(se, w, 1, &mf));
        }
      }
      for (uint32_t w0 = 0; x_phased && (w0 < ks.size()); w0 += chunk) {
        const uint32_t cnt = std::min<uint32_t>(chunk, static_cast<uint32_t>(ks.size()) - w0);
        rows.assign(static_cast<size_t>(cnt) * s_rec, 0);
        mfs.assign(cnt, 0.0);
        const uint32_t nthreads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        std::vector<std::thread> pool;
        for (uint32_t t = 0; t < nthreads; ++t) {
          pool.emplace_back([&, t]() {
            std::vector<uint8_t> raw_row(in_rec + 8), lo_a, hi_a, ph_a;
            for (uint32_t w = t; w < cnt; w += nthreads) {
              const uint32_t raw_v = inc[ks[w0 + w]];
              if (x_phased && (V.alt_ct[raw_v] > 1)) {
                // several ALT alleles: collapsed on the major allele of chrX's allele-frequency rule, the non-males' haplotypes split in Get1MP's reading
                if (lo_a.empty()) {
                  lo_a.resize(raw_sample_ct);
                  hi_a.resize(raw_sample_ct);
                  ph_a.resize(2 * ((static_cast<size_t>(raw_sample_ct) + 7) / 8));
                }
                bool unph = false;
                multiallelic_sex_row_phased(pg, raw_v, V.alt_ct[raw_v], sp, &lo_a, &hi_a, ph_a.data(), ph_a.size() / 2, rows.data() + static_cast<uint64_t>(w) * s_rec, s_rec,
                                            &mfs[w], &unph);
                if (unph) {
                  atomic_min(&x_unphased, raw_v);
                }
                continue;
              }
              if (x_phased) {
                uint32_t at = 0;
                const int prc = ldp_pgen_read_phased(pg, raw_v, 1, raw_row.data(), in_rec, nonmale_mask.data(), 1, &at);
                if (prc == LDP_ERR_UNPHASED) {
                  atomic_min(&x_unphased, raw_v);
                  continue;
                }
                if (prc) {
                  die(6, "\nError: %s\n", ldp_pgen_last_error(pg));
                }
                build_sex_row(sp, raw_row.data(), rows.data() + static_cast<uint64_t>(w) * s_rec, s_rec, &mfs[w], raw_row.data() + in_phase_off);
                continue;
              }
              fetch_raw_row(pg, storage_mode, raw_v, raw_sample_ct, rec_bytes, raw_row.data());
              build_sex_row(sp, raw_row.data(), rows.data() + static_cast<uint64_t>(w) * s_rec, s_rec, &mfs[w]);
            }
          });
        }
        for (std::thread& t : pool) {
          t.join();
        }
        if (x_unphased.load() != UINT32_MAX) {
          die_unphased(x_unphased.load());
        }
        must(se, ldp_load_genotypes(se, w0, cnt, rows.data(), s_rec, LDP_MEM_HOST, LDP_GENO_INVERSE));
        must(se, ldp_set_maj_freqs(se, w0, cnt, mfs.data()));
      }
      const std::vector<uint64_t> pref_s = sub_preferred(ks);
      if (!pref_s.empty()) {
        ldp_set_preferred(se, pref_s.data());
      }
      std::vector<uint64_t> bm((ks.size() + 63) / 64 + 1, 0);
      must(se, ldp_run(se, bm.data()));
      scatter(bm, ks);
      ldp_destroy(se);
    }
  }

  void write_lists() {
    uint32_t removed_ct = 0;
    for (uint64_t w : removed) {
      removed_ct += static_cast<uint32_t>(__builtin_popcountll(w));
    }
    logprintf("%u/%u variants removed.\n", removed_ct, variant_ct);  // plink2_ld.cc:2707
    // LdPruneWrite, plink2_ld.cc:2464-2528
    for (int pass = 0; pass < 2; ++pass) {
      const std::string path = A.out + (pass ? ".prune.out" : ".prune.in");
      FILE* f = fopen(path.c_str(), "wb");
      if (!f) {
        die(3, "Error: Failed to open %s for writing.\n", path.c_str());
      }
      for (uint32_t k = 0; k < variant_ct; ++k) {
        const bool rem = (removed[k >> 6] >> (k & 63)) & 1;
        if (rem == static_cast<bool>(pass)) {
          fputs(V.id[inc[k]].c_str(), f);
          fputc('\n', f);
        }
      }
      if (fclose(f)) {
        die(5, "Error: File write failure: %s.\n", path.c_str());
      }
    }
    logprintf("Variant lists written to %s.prune.in and %s.prune.out .\n", A.out.c_str(), A.out.c_str());
  }

  [[noreturn]] void finish() {
    if (A.timing) {
      // (wall-clock stamps: what a caller's stopwatch sees beyond `total` is process start-up before main() and teardown after _exit)
      const double unix_now = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
      logprintf("[timing] total %.3f s (main() entered at unix time %.3f, leaving at %.3f)\n", now_s() - t_begin, unix_now - (now_s() - t_begin), unix_now);
    }
    if (g_log) {
      fclose(g_log);
    }
    fflush(nullptr);
    // everything is on disk; releasing tens of GB of device memory and unmapping the input only costs time
    _exit(0);
  }

  int run() {
    if ((!A.have_prune) && (!S.report_device) && !((A.het || A.hardy || A.king) && S.device_filter)) {
      if (A.het) {
        het_host_pass(S);  // (the host's filters made the list final in load_inputs)
      }
      if (A.king && !A.dry_run) {
        king_host_pass(S);
      }
      finish();  // a run of reports, of --het or of --make-king-table alone that the host's passes served: no device is touched
    }
    set_params();
    if (A.dry_run) {
      return dry_run();
    }
    if (!S.device_filter) {
      check_unique_ids();
    }
    t_tables_done = now_s();
    plan_engines();
    t_planned = now_s();
    S.join_hip();
    if (ldp_device_count() < 1) {
      die(16, "Error: no usable HIP device (plink2-hip has no CPU compute path).\n");
    }
    removed.assign((static_cast<size_t>(variant_ct) + 63) / 64 + 1, 0);
    if (S.device_filter) {
      // load first, then filter and plan; the ID check and --indep-preferred are about the variants the filters leave
      t_load0 = now_s();
      set_row_geometry();
      t_rows0 = now_s();
      load_diploid_rows();
      t_rows1 = now_s();
      if (S.mind_device && mind_on_device()) {
        return 0;  // (S.restart: main() starts over without the removed samples)
      }
      if (S.report_device) {
        reports_on_device();
        if ((!A.have_prune) && (!A.het) && (!A.hardy) && !A.king) {
          S.file_to_hbm_done();
          finish();  // a run of reports alone stops here: no plan, no pair kernel
        }
      }
      if (A.have_prune || S.count_filters) {
        filter_on_device();
      }
      if (!A.have_prune) {
        report_filter_timing();
        if (A.het) {
          het_stage();  // --het alone, after the filters: no band plan, no pair kernel
        }
        if (A.king) {
          king_stage();  // (the same for --make-king-table, behind --het)
        }
        S.file_to_hbm_done();
        finish();
      }
      check_unique_ids();
    }
    if (subcontig_ct || !xk.empty() || !yk.empty() || !tk.empty()) {
      check_before_loading();
      read_preferred();
      logprintf("--indep-pair%s (%d GPU%s): ", A.pairphase ? "phase" : "wise", world, world == 1 ? "" : "s");
      fflush(stdout);
      if (!S.device_filter) {
        t_load0 = now_s();
      }
      if (A.timing) {
        logprintf("\n[timing] table parse %.3f s, variant-table passes + ID check done at %.3f s, engine planned at %.3f s, HIP init %.3f s (concurrent; joined at %.3f s)\n",
                  t_parse, t_tables_done - t_begin, t_planned - t_begin, t_hip_init, t_joined - t_begin);
        if (S.device_filter) {
          report_filter_timing();  // (the host pass reports itself where it runs: load_inputs)
        }
      }
      if (!S.device_filter) {
        set_row_geometry();
      }
      t_load1 = now_s();
      t_run1 = 0;
      if (subcontig_ct) {
        if (!S.device_filter) {
          t_rows0 = now_s();
          load_diploid_rows();
          t_rows1 = now_s();
        }
        patch_host_built_rows();
        set_dosage_frequencies();
        S.file_to_hbm_done();  // (this thread moved next to device 0 for the file -> HBM leg, Session::join_hip: back to where it was)
        run_diploid_engines();
      }
      if (A.timing) {
        report_load_and_run();
      }
      run_sex_chromosomes();
    }
    write_lists();
    if (A.het) {
      het_stage();  // (right behind LdPrune, plink2.cc:2958; the restricted engine's image is as the filters left it)
    }
    if (A.king) {
      king_stage();
    }
    finish();
  }
};

int run_prune(Session& S) {
  PruneJob job(S);
  return job.run();
}



}  // namespace p2h
