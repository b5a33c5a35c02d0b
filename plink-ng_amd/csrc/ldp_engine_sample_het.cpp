// ldp_engine_sample_het.cpp -- ldp_sample_het_counts(): per-sample het-call counts, missing-call counts and weighted missing-call sums of
// loaded rows, read from the resident 2-bit image (ldp_sample_het.hip).  Contract, states and refusals are those of
// resident_runs() (ldp_engine.cpp), with the image: one launch per run of owned rows.  include / weight are the caller's per-variant arrays of
// the range; each launch gets them from its run's first variant on.
// (host runtime behind include/ldprune_hip.h; ldp_engine.cpp has the overview)
#include "ldp_engine_internal.h"

namespace {

// slab_rows: rows per slab (0: chosen by the launch); ms_kernel / bytes_read (optional): the device time of the launches (HIP events on the
// engine's stream) and the image bytes they read.  The call keeps no state in the engine: what the test hook wants comes back through it.
int sample_het_counts_impl(ldp_engine* e, uint32_t first_variant, uint32_t n, const uint8_t* include, const uint64_t* weight, uint32_t* het_ct, uint32_t* missing_ct,
                           uint64_t* missing_weight, uint32_t slab_rows, double* ms_kernel, uint64_t* bytes_read) {
  if (!e) {
    return LDP_ERR_INVALID;
  }
  if (ms_kernel) {
    *ms_kernel = 0.0;
  }
  if (bytes_read) {
    *bytes_read = 0;
  }
  if (!e->planned) {
    return fail(e, LDP_ERR_STATE, "ldp_set_variants*() and the loads first");
  }
  if (!het_ct || !missing_ct) {
    return fail(e, LDP_ERR_INVALID, "het_ct or missing_ct is NULL");
  }
  if (weight && !missing_weight) {
    return fail(e, LDP_ERR_INVALID, "weight given but missing_weight is NULL");
  }
  std::vector<ResidentRun> runs;
  int rc = resident_runs(e, "ldp_sample_het_counts()", first_variant, n, true, &runs);
  if (rc) {
    return rc;
  }
  const uint32_t founder_ct = e->P.founder_ct;
  memset(het_ct, 0, static_cast<size_t>(founder_ct) * sizeof(uint32_t));
  memset(missing_ct, 0, static_cast<size_t>(founder_ct) * sizeof(uint32_t));
  if (missing_weight) {
    memset(missing_weight, 0, static_cast<size_t>(founder_ct) * sizeof(uint64_t));
  }
  if (!n) {
    return LDP_OK;
  }
  rc = begin_resident_read(e);
  if (rc) {
    return rc;
  }
  // one allocation: missing_weight | weight (64-bit), het_ct | missing_ct (32-bit), include (bytes)
  const size_t fc = founder_ct;
  const size_t off_w = fc * 8, off_het = off_w + (weight ? static_cast<size_t>(n) * 8 : 0), off_mis = off_het + fc * 4, off_inc = off_mis + fc * 4;
  const size_t total = off_inc + (include ? n : 0);
  DevBuf d_all;
  EventSet<2> ev;
  HIP_TRY(e, ev.create());
  HIP_TRY(e, hipMalloc(&d_all.p, total));
  uint8_t* base = d_all.as<uint8_t>();
  uint64_t* d_mw = reinterpret_cast<uint64_t*>(base);
  uint64_t* d_weight = weight ? reinterpret_cast<uint64_t*>(base + off_w) : nullptr;
  uint32_t* d_het = reinterpret_cast<uint32_t*>(base + off_het);
  uint32_t* d_mis = reinterpret_cast<uint32_t*>(base + off_mis);
  uint8_t* d_inc = include ? base + off_inc : nullptr;
  HIP_TRY(e, hipMemsetAsync(d_mw, 0, fc * 8, e->stream));
  HIP_TRY(e, hipMemsetAsync(d_het, 0, fc * 8, e->stream));  // het_ct and missing_ct
  if (weight) {
    HIP_TRY(e, hipMemcpyAsync(d_weight, weight, static_cast<size_t>(n) * 8, hipMemcpyHostToDevice, e->stream));
  }
  if (include) {
    HIP_TRY(e, hipMemcpyAsync(d_inc, include, n, hipMemcpyHostToDevice, e->stream));
  }
  HIP_TRY(e, hipEventRecord(ev.ev[0], e->stream));
  uint64_t bytes = 0;
  for (const ResidentRun& r : runs) {
    const hipError_t krc = launch_sample_het(e->d_codes, e->code_row_bytes, r.l_first, r.ct, founder_ct, d_inc ? d_inc + r.off : nullptr, d_weight ? d_weight + r.off : nullptr, d_het,
                                             d_mis, d_weight ? d_mw : nullptr, slab_rows, e->stream);
    if (krc != hipSuccess) {
      return hipfail(e, krc, "sample_het_kernel launch");
    }
    bytes += static_cast<uint64_t>(r.ct) * e->code_row_bytes;
  }
  HIP_TRY(e, hipEventRecord(ev.ev[1], e->stream));
  HIP_TRY(e, hipMemcpyAsync(het_ct, d_het, fc * 4, hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(e, hipMemcpyAsync(missing_ct, d_mis, fc * 4, hipMemcpyDeviceToHost, e->stream));
  if (weight) {
    HIP_TRY(e, hipMemcpyAsync(missing_weight, d_mw, fc * 8, hipMemcpyDeviceToHost, e->stream));
  }
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  if (ms_kernel) {
    *ms_kernel = ev.elapsed_ms(0, 1);
  }
  if (bytes_read) {
    *bytes_read = bytes;
  }
  return LDP_OK;
}

}  // namespace

extern "C" {

int ldp_sample_het_counts(ldp_engine* e, uint32_t first_variant, uint32_t n, const uint8_t* include, const uint64_t* weight, uint32_t* het_ct, uint32_t* missing_ct,
                          uint64_t* missing_weight) {
  return sample_het_counts_impl(e, first_variant, n, include, weight, het_ct, missing_ct, missing_weight, 0, nullptr, nullptr);
}

int ldp_debug_sample_het_counts(ldp_engine* e, uint32_t first_variant, uint32_t n, const uint8_t* include, const uint64_t* weight, uint32_t* het_ct, uint32_t* missing_ct,
                                uint64_t* missing_weight, uint32_t slab_rows, double* ms_kernel, uint64_t* bytes_read) {
  return sample_het_counts_impl(e, first_variant, n, include, weight, het_ct, missing_ct, missing_weight, slab_rows, ms_kernel, bytes_read);
}

}  // extern "C"
