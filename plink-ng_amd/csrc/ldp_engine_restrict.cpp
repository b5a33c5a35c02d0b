// ldp_engine_restrict.cpp -- ldp_restrict_variants(): load first, then drop variants and plan.  The resident image is compacted where it
// lies (ldp_compact.hip, in the batches of ldp_compact_schedule.h), the engine is planned again over the kept variants by the code
// ldp_set_variants() runs, and everything it keeps per row arrives at the row's new index ("restricting a loaded engine"):
//   image rows, d_stored_inv                     compacted with the index array
//   maj_freq / mf_set / loaded / preferred bits  compacted on the host (they live there)
//   code-image engines: d_recs, d_cp_stats       recomputed: the count pass runs over the compacted rows in place (the ldp_map_rows +
//                                                LDP_MEM_DEVICE path), with the NEW plan's checkpoints
//   bit-plane engines: d_recs, d_cp_stats, d_cp_gen  compacted with the index array (their count pass reads input rows, not planes);
//                                                the engine keeps the checkpoints those statistics were counted for
//   plan-sized arrays (band, predicate rows, work plans, route words, missing-call statistics of the launches)  reallocated, filled when launches are queued
// (host runtime behind include/ldprune_hip.h; ldp_engine.cpp has the overview)
#include "ldp_engine_internal.h"
#include "ldp_compact_schedule.h"

extern "C" {

int ldp_restrict_variants(ldp_engine* e, const uint64_t* keep_bitmap, uint32_t kept_ct, const uint32_t* chr_idx, const uint32_t* bps) {
  if (!e) {
    return LDP_ERR_INVALID;
  }
  if (!e->planned) {
    return fail(e, LDP_ERR_STATE, "ldp_set_variants*() and the loads first");
  }
  if (e->world > 1) {
    return fail(e, LDP_ERR_UNSUPPORTED, "ldp_restrict_variants() on a sharded engine (ldp_set_shard with world > 1)");
  }
  if (e->loaded_special) {
    return fail(e, LDP_ERR_UNSUPPORTED, "ldp_restrict_variants() on rows loaded as LDP_GENO_PHASED or through a sample map that is no plain subset of the file's samples");
  }
  const uint32_t old_ct = e->variant_ct;
  if ((old_ct && !keep_bitmap) || (kept_ct > old_ct)) {
    return fail(e, LDP_ERR_INVALID, "keep_bitmap is NULL or kept_ct exceeds the variant count");
  }
  if (kept_ct && !chr_idx) {
    return fail(e, LDP_ERR_INVALID, "chr_idx is NULL");
  }
  if (e->P.window_is_bp && kept_ct && !bps) {
    return fail(e, LDP_ERR_INVALID, "bp-based window needs variant positions");
  }
  std::vector<uint32_t> kept;  // old global index of kept variant k
  kept.reserve(kept_ct);
  for (uint32_t v = 0; v < old_ct; ++v) {
    if ((keep_bitmap[v >> 6] >> (v & 63)) & 1) {
      if (kept.size() == kept_ct) {
        return fail(e, LDP_ERR_INVALID, "keep_bitmap has more bits set than kept_ct");
      }
      kept.push_back(v);
    }
  }
  if (kept.size() != kept_ct) {
    return fail(e, LDP_ERR_INVALID, "keep_bitmap has fewer bits set than kept_ct");
  }
  for (uint32_t v = 1; v < kept_ct; ++v) {  // (what ldp_set_variants() checks, before anything is changed)
    if (chr_idx[v] < chr_idx[v - 1]) {
      return fail(e, LDP_ERR_INVALID, "chr_idx must be nondecreasing");
    }
    if (e->P.window_is_bp && (chr_idx[v] == chr_idx[v - 1]) && (bps[v] < bps[v - 1])) {
      return fail(e, LDP_ERR_INVALID, "positions must be sorted within a chromosome (plink2.cc:2926)");
    }
  }
  // ---- the state the call starts from: every owned row loaded, no pair work queued
  if (!e->plan_uploaded) {
    return fail(e, LDP_ERR_STATE, "nothing is loaded");
  }
  for (uint32_t l = 0; l < e->local_ct; ++l) {
    if (!e->loaded[l]) {
      return fail(e, LDP_ERR_STATE, "genotypes missing for an owned variant (ldp_load_genotypes)");
    }
  }
  bool queued = (e->next_group != 0) || e->pred_valid;
  for (int k = 0; k < kPairStreams; ++k) {
    queued = queued || e->pair_tail_set[k];
  }
  if (queued) {
    return fail(e, LDP_ERR_STATE, "pair work has been queued on these rows (load through ldp_set_variants_matrix(), restrict, then run)");
  }
  // ---- which old row each row of the restricted engine comes from: the owned variants of the new plan, in order
  std::vector<Subcontig> new_subs;
  uint32_t new_window_max = 0;
  subcontig_split(chr_idx, e->P.window_is_bp ? bps : nullptr, kept_ct, e->P.prune_window_size, &new_subs, &new_window_max);
  std::vector<uint32_t> src;  // new local row -> old local row
  for (const Subcontig& s : new_subs) {
    for (uint32_t v = 0; v < s.len; ++v) {
      const int64_t l = e->global_to_local[kept[s.first + v]];
      if (l < 0) {
        return fail(e, LDP_ERR_STATE, "a kept variant has no row in this engine (its plan did not own it)");
      }
      src.push_back(static_cast<uint32_t>(l));
    }
  }
  const uint32_t new_local = static_cast<uint32_t>(src.size());
  for (uint32_t k = 0; k < new_local; ++k) {
    if ((src[k] < k) || (k && (src[k] <= src[k - 1]))) {
      return fail(e, LDP_ERR_STATE, "internal: the kept rows are not in ascending order");
    }
  }
  // the host's per-row state at the new indices
  std::vector<double> new_mf(new_local);
  std::vector<uint8_t> new_mf_set(new_local), new_inv(new_local);
  std::vector<uint64_t> new_dos_ref(new_local), new_dos_alt(new_local);
  std::vector<uint8_t> new_dos_has(new_local);
  std::vector<std::vector<uint32_t>> new_allele_cts(new_local);
  bool any_inv = false;
  for (uint32_t k = 0; k < new_local; ++k) {
    new_dos_ref[k] = e->dos_ref[src[k]];
    new_dos_alt[k] = e->dos_alt[src[k]];
    new_dos_has[k] = e->dos_has[src[k]];
    new_allele_cts[k] = e->allele_cts[src[k]];
    new_mf[k] = e->maj_freq[src[k]];
    new_mf_set[k] = e->mf_set[src[k]];
    new_inv[k] = e->row_inv_loaded[src[k]];
    any_inv = any_inv || new_inv[k];
  }
  std::vector<uint64_t> new_preferred;
  if (!e->preferred.empty()) {
    new_preferred.assign((static_cast<size_t>(kept_ct) + 63) / 64, 0);
    for (uint32_t k = 0; k < kept_ct; ++k) {
      if ((e->preferred[kept[k] >> 6] >> (kept[k] & 63)) & 1) {
        new_preferred[k >> 6] |= 1ull << (k & 63);
      }
    }
  }
  HIP_TRY(e, hipSetDevice(e->device));
  // everything queued so far (the count pass, the copy of the records) is finished before rows move
  HIP_TRY(e, hipStreamSynchronize(e->copy_stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  const bool codes = e->codes_format;
  const uint64_t pitch = codes ? e->code_row_bytes : e->row_dwords * sizeof(uint32_t);
  uint8_t* image = codes ? e->d_codes : reinterpret_cast<uint8_t*>(e->d_planes);
  // ---- the image, where it lies
  uint32_t batch_rows = e->opt.compact_batch_rows;
  if (!batch_rows) {
    batch_rows = static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>((256ull << 20) / pitch, 1), 0xffffffffull));
  }
  batch_rows = static_cast<uint32_t>(std::min<uint64_t>(batch_rows, std::max<uint64_t>(((1ull << 35) / pitch), 1)));  // (one launch: below 2^31 16-byte units)
  std::vector<CompactBatch> sched;
  compact_schedule(src.data(), new_local, batch_rows, &sched);
  DevBuf d_src, d_bounce, d_inv_new, d_row_inverse, old_recs, old_cp, old_cp_gen;
  EventSet<2> ev;
  HIP_TRY(e, ev.create());
  uint64_t moved = 0, direct = 0, bounced = 0;
  if (new_local) {
    HIP_TRY(e, hipMalloc(&d_src.p, static_cast<size_t>(new_local) * sizeof(uint32_t)));
    HIP_TRY(e, hipMemcpyAsync(d_src.p, src.data(), static_cast<size_t>(new_local) * sizeof(uint32_t), hipMemcpyHostToDevice, e->stream));
  }
  uint8_t* bounce = nullptr;
  uint32_t bounce_rows = 0;
  for (const CompactBatch& b : sched) {
    if (b.bounce) {
      bounce_rows = std::max(bounce_rows, b.k1 - b.k0);
    }
  }
  if (bounce_rows) {
    const size_t need = static_cast<size_t>(bounce_rows) * pitch;
    for (int k = 0; k < ldp_engine::kDecSlots; ++k) {  // (the decode scratch of ldp_load_pgen_records(), when it is there and large enough: its contents are per launch)
      if (e->dec.ptr[k] && (e->dec.cap[k] >= need)) {
        bounce = static_cast<uint8_t*>(e->dec.ptr[k]);
        break;
      }
    }
    if (!bounce) {
      HIP_TRY(e, hipMalloc(&d_bounce.p, need));
      bounce = d_bounce.as<uint8_t>();
    }
  }
  HIP_TRY(e, hipEventRecord(ev.ev[0], e->stream));
  for (const CompactBatch& b : sched) {
    const uint32_t rows = b.k1 - b.k0;
    const uint32_t* idx = d_src.as<uint32_t>() + b.k0;
    hipError_t krc;
    if (b.bounce) {
      krc = launch_compact_rows(bounce, image, pitch, idx, 0, rows, e->stream);
      if (krc == hipSuccess) {
        krc = launch_compact_rows(image, bounce, pitch, nullptr, b.k0, rows, e->stream);
      }
      bounced += rows;
    } else {
      krc = launch_compact_rows(image, image, pitch, idx, b.k0, rows, e->stream);
      direct += rows;
    }
    if (krc != hipSuccess) {
      return hipfail(e, krc, "compact_rows_kernel launch");
    }
    moved += rows;
  }
  HIP_TRY(e, hipEventRecord(ev.ev[1], e->stream));
  if (codes && new_local) {
    // the row flags the in-place count pass reads (out of place: one byte per row)
    HIP_TRY(e, hipMalloc(&d_inv_new.p, std::max<size_t>(new_local, 1)));
    const hipError_t grc = launch_gather_bytes(d_inv_new.as<uint8_t>(), e->d_stored_inv, d_src.as<uint32_t>(), new_local, e->stream);
    if (grc != hipSuccess) {
      return hipfail(e, grc, "gather_bytes_kernel launch");
    }
    HIP_TRY(e, hipMemcpyAsync(e->d_stored_inv, d_inv_new.p, new_local, hipMemcpyDeviceToDevice, e->stream));
  }
  if (!codes) {
    // bit-plane engines: the records and checkpoint statistics travel with their rows (gathered into the new arrays below)
    old_recs.p = e->d_recs;
    old_cp.p = e->d_cp_stats;
    old_cp_gen.p = e->d_cp_gen;
    e->d_recs = nullptr;
    e->d_cp_stats = nullptr;
    e->d_cp_gen = nullptr;
    if (!e->cp_frozen) {
      e->frozen_n_checkpoints = e->n_checkpoints;
      for (int k = 0; k < kCheckpoints; ++k) {
        e->frozen_cp_chunk[k] = e->checkpoint_chunk[k];
      }
    }
  }
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  e->rows_compacted = moved;
  e->rows_direct = direct;
  e->rows_bounced = bounced;
  e->ms_compact = ev.elapsed_ms(0, 1);
  // ---- plan again: the plan-sized arrays go, the image stays (its tail is unused until ldp_release_device())
  free_device(e, true);
  if (!codes) {
    e->cp_frozen = true;
  }
  e->replan_keeps_image = true;
  int rc = ldp_set_variants(e, kept_ct, chr_idx, bps);
  e->replan_keeps_image = false;
  if (rc) {
    return rc;
  }
  if (e->local_ct != new_local) {
    return fail(e, LDP_ERR_STATE, "internal: the plan owns other rows than the compaction moved");
  }
  rc = ensure_device_plan(e);
  if (rc) {
    return rc;
  }
  if (!new_preferred.empty()) {
    e->preferred.swap(new_preferred);
  } else {
    e->preferred.clear();
  }
  if (codes) {
    // records, orientation flags and checkpoint statistics from the rows themselves, under the new plan
    if (any_inv) {
      HIP_TRY(e, hipMalloc(&d_row_inverse.p, new_local));
      HIP_TRY(e, hipMemcpyAsync(d_row_inverse.p, new_inv.data(), new_local, hipMemcpyHostToDevice, e->stream));
    }
    for (const ldp_engine::OwnedRun& r : e->owned_runs) {
      const uint32_t l0 = static_cast<uint32_t>(e->global_to_local[r.g_first]);
      rc = load_rows_impl(e, r.g_first, r.g_end - r.g_first, e->d_codes + static_cast<uint64_t>(l0) * pitch, pitch, LDP_MEM_DEVICE, LDP_GENO_REF,
                          any_inv ? (d_row_inverse.as<uint8_t>() + l0) : nullptr, any_inv ? (new_inv.data() + l0) : nullptr, -1, 0);
      if (rc) {
        return rc;
      }
    }
  } else if (new_local) {
    hipError_t krc = launch_compact_rows(e->d_recs, old_recs.p, sizeof(ldp_variant_rec), d_src.as<uint32_t>(), 0, new_local, e->stream);
    if (krc == hipSuccess) {
      krc = launch_compact_rows(e->d_cp_stats, old_cp.p, kCpStride * sizeof(cp_slot), d_src.as<uint32_t>(), 0, new_local, e->stream);
    }
    if (krc == hipSuccess) {
      krc = launch_compact_rows(e->d_cp_gen, old_cp_gen.p, kCheckpoints * sizeof(cp_gen_slot), d_src.as<uint32_t>(), 0, new_local, e->stream);
    }
    if (krc != hipSuccess) {
      return hipfail(e, krc, "compact_rows_kernel launch (records)");
    }
    std::fill(e->loaded.begin(), e->loaded.end(), static_cast<uint8_t>(1));
    std::fill(e->load_tag.begin(), e->load_tag.end(), e->load_epoch);
    e->row_inv_loaded = new_inv;
    e->recs_host_valid = false;
    e->recs_copy_queued = false;
  }
  // frequencies: a caller's own stay (ldp_set_maj_freqs, collapsed multiallelic rows), the others are derived from the records again
  for (uint32_t k = 0; k < new_local; ++k) {
    if (new_mf_set[k] == 1) {
      e->maj_freq[k] = new_mf[k];
      e->mf_set[k] = 1;
    } else if (!codes) {
      e->maj_freq[k] = new_mf[k];
      e->mf_set[k] = new_mf_set[k] ? 2 : 0;
    }
  }
  // the dosage sums are sums over a row's samples: they travel with it
  e->dos_ref.swap(new_dos_ref);
  e->dos_alt.swap(new_dos_alt);
  e->dos_has.swap(new_dos_has);
  e->allele_cts.swap(new_allele_cts);  // (... and so do a multiallelic row's allele counts)
  HIP_TRY(e, hipStreamSynchronize(e->stream));  // (the temporaries above are read until here)
  return LDP_OK;
}

int ldp_debug_get_compact_stats(const ldp_engine* e, uint64_t* rows_compacted, uint64_t* rows_direct, uint64_t* rows_bounced, double* ms_compact) {
  if (!e) {
    return LDP_ERR_INVALID;
  }
  if (rows_compacted) {
    *rows_compacted = e->rows_compacted;
  }
  if (rows_direct) {
    *rows_direct = e->rows_direct;
  }
  if (rows_bounced) {
    *rows_bounced = e->rows_bounced;
  }
  if (ms_compact) {
    *ms_compact = e->ms_compact;
  }
  return LDP_OK;
}

}  // extern "C"
