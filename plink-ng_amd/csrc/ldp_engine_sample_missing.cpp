// ldp_engine_sample_missing.cpp -- ldp_sample_missing_counts(): per-sample missing-call counts of loaded rows, read from the resident
// 2-bit image (ldp_sample_missing.hip).  Contract, states and refusals are those of resident_runs() (ldp_engine.cpp),
// with the image: nothing of the engine changes, and the requested variants are walked as the runs of consecutive image rows the engine owns
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
  std::vector<ResidentRun> runs;
  int rc = resident_runs(e, "ldp_sample_missing_counts()", first_variant, n, true, &runs);
  if (rc) {
    return rc;
  }
  const uint32_t founder_ct = e->P.founder_ct;
  e->ms_sample_missing = 0.0;
  e->sample_missing_bytes = 0;
  memset(out, 0, static_cast<size_t>(founder_ct) * sizeof(uint32_t));
  if (!n) {
    return LDP_OK;
  }
  rc = begin_resident_read(e);
  if (rc) {
    return rc;
  }
  DevBuf d_counts;
  EventSet<2> ev;
  HIP_TRY(e, ev.create());
  HIP_TRY(e, hipMalloc(&d_counts.p, static_cast<size_t>(founder_ct) * sizeof(uint32_t)));
  HIP_TRY(e, hipMemsetAsync(d_counts.p, 0, static_cast<size_t>(founder_ct) * sizeof(uint32_t), e->stream));
  HIP_TRY(e, hipEventRecord(ev.ev[0], e->stream));
  for (const ResidentRun& r : runs) {
    const hipError_t krc = launch_sample_missing(e->d_codes, e->code_row_bytes, r.l_first, r.ct, founder_ct, d_counts.as<uint32_t>(), e->opt.sample_missing_slab_rows, e->stream);
    if (krc != hipSuccess) {
      return hipfail(e, krc, "sample_missing_kernel launch");
    }
    e->sample_missing_bytes += static_cast<uint64_t>(r.ct) * e->code_row_bytes;
  }
  HIP_TRY(e, hipEventRecord(ev.ev[1], e->stream));
  HIP_TRY(e, hipMemcpyAsync(out, d_counts.p, static_cast<size_t>(founder_ct) * sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  e->ms_sample_missing = ev.elapsed_ms(0, 1);
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
