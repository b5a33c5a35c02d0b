// ldp_engine_hwe.cpp -- ldp_hwe_ln_pvals(): the exact Hardy-Weinberg test of loaded rows, from the genotype counts the count pass left in the
// records on the device (hwe_kernel, ldp_hwe.hip), and ldp_hwe_ln_pvals_counts(), the same kernel on counts from
// anywhere.  Contract, states and refusals of the engine call are those of resident_runs() (ldp_engine.cpp; one launch per run of owned
// records), with three deviations marked below: the image is not read, so engines that keep bit-planes are served too; the records have to
// be on the device; and a row whose record carries no raw counts (loaded as LDP_GENO_INVERSE) is refused.
// (host runtime behind include/ldprune_hip.h; ldp_engine.cpp has the overview)
#include "ldp_engine_internal.h"

namespace {

int hwe_ln_pvals_impl(ldp_engine* e, uint32_t first_variant, uint32_t n, int midp, double* ln_p, uint8_t* flags, double* ms_kernel) {
  if (!e) {
    return LDP_ERR_INVALID;
  }
  if (ms_kernel) {
    *ms_kernel = 0.0;
  }
  if (!e->planned) {
    return fail(e, LDP_ERR_STATE, "ldp_set_variants*() and the loads first");
  }
  if (!ln_p) {
    return fail(e, LDP_ERR_INVALID, "ln_p is NULL");
  }
  // HWE's own: the records are read, not the image, so an engine that keeps bit-planes is served (no needs_image)
  std::vector<ResidentRun> runs;
  int rc = resident_runs(e, "ldp_hwe_ln_pvals()", first_variant, n, false, &runs);
  if (rc) {
    return rc;
  }
  // HWE's own: what is read are the records of the device-side plan
  if (n && !e->d_recs) {
    return fail(e, LDP_ERR_STATE, "nothing is loaded");
  }
  // HWE's own: the record of a row that came inverted holds no raw genotype counts
  for (const ResidentRun& r : runs) {
    for (uint32_t l = r.l_first; l < r.l_first + r.ct; ++l) {
      if (e->row_inv_loaded[l]) {
        return fail(e, LDP_ERR_UNSUPPORTED, "ldp_hwe_ln_pvals() on a row loaded as LDP_GENO_INVERSE (its record carries no genotype counts)");
      }
    }
  }
  if (!n) {
    return LDP_OK;
  }
  rc = begin_resident_read(e);
  if (rc) {
    return rc;
  }
  // one allocation: ln_p (64-bit) | flags (bytes)
  const size_t off_flags = static_cast<size_t>(n) * 8;
  DevBuf d_all;
  EventSet<2> ev;
  HIP_TRY(e, ev.create());
  HIP_TRY(e, hipMalloc(&d_all.p, off_flags + n));
  double* d_ln = d_all.as<double>();
  uint8_t* d_flags = d_all.as<uint8_t>() + off_flags;
  HIP_TRY(e, hipEventRecord(ev.ev[0], e->stream));
  for (const ResidentRun& r : runs) {
    const hipError_t krc = launch_hwe(e->d_recs + r.l_first, nullptr, nullptr, nullptr, r.ct, midp ? 1 : 0, d_ln + r.off, d_flags + r.off, e->stream);
    if (krc != hipSuccess) {
      return hipfail(e, krc, "hwe_kernel launch");
    }
  }
  HIP_TRY(e, hipEventRecord(ev.ev[1], e->stream));
  HIP_TRY(e, hipMemcpyAsync(ln_p, d_ln, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost, e->stream));
  if (flags) {
    HIP_TRY(e, hipMemcpyAsync(flags, d_flags, n, hipMemcpyDeviceToHost, e->stream));
  }
  HIP_TRY(e, hipStreamSynchronize(e->stream));
  if (ms_kernel) {
    *ms_kernel = ev.elapsed_ms(0, 1);
  }
  return LDP_OK;
}

// a stream of the call's own, released on every exit path
struct OwnStream {
  hipStream_t s = nullptr;
  ~OwnStream() {
    if (s) {
      (void)hipStreamDestroy(s);
    }
  }
};

int hwe_ln_pvals_counts_impl(int device, uint32_t n, const uint32_t* hom1, const uint32_t* het, const uint32_t* hom2, int midp, double* ln_p, uint8_t* flags, double* ms_kernel) {
  if (ms_kernel) {
    *ms_kernel = 0.0;
  }
  if (n && (!hom1 || !het || !hom2 || !ln_p)) {
    return LDP_ERR_INVALID;
  }
  for (uint32_t v = 0; v < n; ++v) {
    if (static_cast<uint64_t>(hom1[v]) + het[v] + hom2[v] >= (1ull << 31)) {
      return LDP_ERR_INVALID;
    }
  }
  if (!n) {
    return LDP_OK;
  }
  if (device >= 0) {
    if (hipSetDevice(device) != hipSuccess) {
      (void)hipGetLastError();
      return LDP_ERR_GPU;
    }
  }
#define HWE_TRY(call)                   \
  do {                                  \
    if ((call) != hipSuccess) {         \
      (void)hipGetLastError();          \
      return LDP_ERR_GPU;               \
    }                                   \
  } while (0)
  OwnStream st;
  DevBuf d_all;
  EventSet<2> ev;
  HWE_TRY(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
  HWE_TRY(ev.create());
  // one allocation: ln_p (64-bit) | hom1 | het | hom2 (32-bit) | flags (bytes)
  const size_t cnt = n, off_cts = cnt * 8, off_flags = off_cts + 3 * cnt * 4;
  HWE_TRY(hipMalloc(&d_all.p, off_flags + cnt));
  uint8_t* base = d_all.as<uint8_t>();
  double* d_ln = reinterpret_cast<double*>(base);
  uint32_t* d_cts = reinterpret_cast<uint32_t*>(base + off_cts);
  uint8_t* d_flags = base + off_flags;
  HWE_TRY(hipMemcpyAsync(d_cts, hom1, cnt * 4, hipMemcpyHostToDevice, st.s));
  HWE_TRY(hipMemcpyAsync(d_cts + cnt, het, cnt * 4, hipMemcpyHostToDevice, st.s));
  HWE_TRY(hipMemcpyAsync(d_cts + 2 * cnt, hom2, cnt * 4, hipMemcpyHostToDevice, st.s));
  HWE_TRY(hipEventRecord(ev.ev[0], st.s));
  HWE_TRY(launch_hwe(nullptr, d_cts, d_cts + cnt, d_cts + 2 * cnt, n, midp ? 1 : 0, d_ln, d_flags, st.s));
  HWE_TRY(hipEventRecord(ev.ev[1], st.s));
  HWE_TRY(hipMemcpyAsync(ln_p, d_ln, cnt * 8, hipMemcpyDeviceToHost, st.s));
  if (flags) {
    HWE_TRY(hipMemcpyAsync(flags, d_flags, cnt, hipMemcpyDeviceToHost, st.s));
  }
  HWE_TRY(hipStreamSynchronize(st.s));
#undef HWE_TRY
  if (ms_kernel) {
    *ms_kernel = ev.elapsed_ms(0, 1);
  }
  return LDP_OK;
}

}  // namespace

extern "C" {

int ldp_hwe_ln_pvals(ldp_engine* e, uint32_t first_variant, uint32_t n, int midp, double* ln_p, uint8_t* flags) {
  return hwe_ln_pvals_impl(e, first_variant, n, midp, ln_p, flags, nullptr);
}

int ldp_debug_hwe_ln_pvals(ldp_engine* e, uint32_t first_variant, uint32_t n, int midp, double* ln_p, uint8_t* flags, double* ms_kernel) {
  return hwe_ln_pvals_impl(e, first_variant, n, midp, ln_p, flags, ms_kernel);
}

int ldp_hwe_ln_pvals_counts(int device, uint32_t n, const uint32_t* hom1, const uint32_t* het, const uint32_t* hom2, int midp, double* ln_p, uint8_t* flags) {
  return hwe_ln_pvals_counts_impl(device, n, hom1, het, hom2, midp, ln_p, flags, nullptr);
}

int ldp_debug_hwe_ln_pvals_counts(int device, uint32_t n, const uint32_t* hom1, const uint32_t* het, const uint32_t* hom2, int midp, double* ln_p, uint8_t* flags,
                                  double* ms_kernel) {
  return hwe_ln_pvals_counts_impl(device, n, hom1, het, hom2, midp, ln_p, flags, ms_kernel);
}

}  // extern "C"
