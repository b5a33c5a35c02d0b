// ldp_engine_sample_missing.cpp -- ldp_sample_missing_counts(): per-sample missing-call counts of loaded rows, read from the resident
// 2-bit image (ldp_sample_missing.hip).  Nothing of the engine changes: the rows, their records and the plan stay as
// they are, before as after ldp_restrict_variants().  The requested variants are walked as the runs of consecutive image rows the engine owns
// them in (one launch per run: one for every engine loaded under ldp_set_variants_matrix()).
// (host runtime behind include/ldprune_hip.h; ldp_engine.cpp has the overview)
#include "ldp_engine_internal.h"

extern "C" {

int ldp_sample_missing_counts(ldp_engine* e, uint32_t first_variant, uint32_t n, uint32_t* out) {
  if (!e) {
    return LDP_ERR_INVALID;
  }
  if (!e->planned) {
    return fail(e, LDP_ERR_STATE, "ldp_set_variants*() and the loads first");
  }
  if (!out) {
    return fail(e, LDP_ERR_INVALID, "out is NULL");
  }
  if (static_cast<uint64_t>(first_variant) + n > e->variant_ct) {
    return fail(e, LDP_ERR_INVALID, "variant range out of bounds");
  }
  if (e->world > 1) {
    return fail(e, LDP_ERR_UNSUPPORTED, "ldp_sample_missing_counts() on a sharded engine (ldp_set_shard with world > 1)");
  }
  if ((e->P.founder_ct > kMfMaxFounders) || !e->opt.pair_mfma || (e->plan_uploaded && !e->codes_format)) {
    return fail(e, LDP_ERR_UNSUPPORTED, "ldp_sample_missing_counts() on an engine that keeps bit-planes (no 2-bit code image)");
  }
  if (e->loaded_special) {
    return fail(e, LDP_ERR_UNSUPPORTED, "ldp_sample_missing_counts() on rows loaded as LDP_GENO_PHASED or through a sample map that makes het calls missing");
  }
  const uint32_t end = first_variant + n;
  struct Run {
    uint32_t l_first, ct;
  };
  std::vector<Run> runs;
  uint32_t covered = 0;
  for (const ldp_engine::OwnedRun& r : e->owned_runs) {
    const uint32_t a = std::max(r.g_first, first_variant), b = std::min(r.g_end, end);
    if (a < b) {
      runs.push_back({static_cast<uint32_t>(e->global_to_local[a]), b - a});
      covered += b - a;
    }
  }
  if (covered != n) {
    return fail(e, LDP_ERR_STATE, "a variant of the range has no row in this engine (its plan did not own it)");
  }
  if (n && !e->plan_uploaded) {
    return fail(e, LDP_ERR_STATE, "nothing is loaded");
  }
  for (const Run& r : runs) {
    for (uint32_t l = r.l_first; l < r.l_first + r.ct; ++l) {
      if (!e->loaded[l]) {
        return fail(e, LDP_ERR_STATE, "genotypes missing for a variant of the range (ldp_load_genotypes)");
      }
    }
  }
  const uint32_t founder_ct = e->P.founder_ct;
  e->ms_sample_missing = 0.0;
  e->sample_missing_bytes = 0;
  memset(out, 0, static_cast<size_t>(founder_ct) * sizeof(uint32_t));
  if (!n) {
    return LDP_OK;
  }
  HIP_TRY(e, hipSetDevice(e->device));
  // the count pass of the loads (it writes each row's padding, and inverts ALT-major rows) is finished before the rows are read
  HIP_TRY(e, hipStreamSynchronize(e->copy_stream));
  DevBuf d_counts;
  EventSet<2> ev;
  HIP_TRY(e, ev.create());
  HIP_TRY(e, hipMalloc(&d_counts.p, static_cast<size_t>(founder_ct) * sizeof(uint32_t)));
  HIP_TRY(e, hipMemsetAsync(d_counts.p, 0, static_cast<size_t>(founder_ct) * sizeof(uint32_t), e->stream));
  HIP_TRY(e, hipEventRecord(ev.ev[0], e->stream));
  for (const Run& r : runs) {
    const hipError_t krc = launch_sample_missing(e->d_codes, e->code_row_bytes, r.l_first, r.ct, founder_ct, d_counts.as<uint32_t>(), e->opt.sample_missing_slab_rows, e->stream);
    if (krc != hipSuccess) {
      return hipfail(e, krc, "sample_missing_kernel launch");
    }
    e->sample_missing_bytes += static_cast<uint64_t>(r.ct) * e->code_row_bytes;
  }
  HIP_TRY(e, hipEventRecord(ev.ev[1], e->stream));
  HIP_TRY(e, hipMemcpyAsync(out, d_counts.p, static_cast<size_t>(founder_ct) * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, ev.ev[0], ev.ev[1]) != hipSuccess) {
    (void)hipGetLastError();
    ms = 0.f;
  }
  e->ms_sample_missing = ms;
  return LDP_OK;
}

int ldp_debug_get_sample_missing_stats(const ldp_engine* e, double* ms_kernel, uint64_t* bytes_read) {
  if (!e) {
    return LDP_ERR_INVALID;
  }
  if (ms_kernel) {
    *ms_kernel = e->ms_sample_missing;
  }
  if (bytes_read) {
    *bytes_read = e->sample_missing_bytes;
  }
  return LDP_OK;
}

}  // extern "C"
