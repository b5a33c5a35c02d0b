// ldp_hwe.hip -- hwe_kernel: the exact Hardy-Weinberg test of every variant of a launch, ln p in FP64 (ldp_hwe_ln_pvals(),
// ldp_hwe_ln_pvals_counts(); what a host's --hwe / --hardy decide and print from).  One lane per variant, 256-thread
// blocks, grid ceil(n / 256); no LDS, no atomics.  A lane reads its three counts -- from the records the count pass left on the device
// (n_homref, n_het, n_homalt of ldp_variant_rec) or from three arrays --, runs the walk of ldp_hwe_core.h and writes one double and one flag
// byte.  The walk's two loops have integer trip counts (at most min(hom1, hom2) and het / 2 steps); a lane's work is O(sqrt(rare)) for a
// variant near equilibrium and O(rare) at worst (an all-het row), and the lanes of a wave wait for the longest of them: accepted (measured:
// profiles/hwe.md; neither sorted lanes nor a jump to the mode).  A triple that sums to 2^31 or more is not walked: ln p = NaN, flag bit 7.
#include "ldp_device.h"
#include "ldp_hwe_core.h"

namespace ldp {

namespace {

constexpr int kHweThreads = 256;

__global__ __launch_bounds__(kHweThreads) void hwe_kernel(const ldp_variant_rec* __restrict__ recs, const uint32_t* __restrict__ hom1, const uint32_t* __restrict__ het,
                                                           const uint32_t* __restrict__ hom2, uint32_t n, int midp, double* __restrict__ ln_p, uint8_t* __restrict__ flags) {
  const uint32_t v = blockIdx.x * kHweThreads + threadIdx.x;
  if (v >= n) {
    return;
  }
  uint32_t a, b, c;
  if (recs) {
    a = recs[v].n_homref;
    b = recs[v].n_het;
    c = recs[v].n_homalt;
  } else {
    a = hom1[v];
    b = het[v];
    c = hom2[v];
  }
  uint8_t f = 0;
  double r;
  if (static_cast<uint64_t>(a) + b + c >= (1ull << 31)) {
    r = __longlong_as_double(0x7ff8000000000000ll);
    f = kHweFlagInvalid;
  } else {
    r = ldp_hwe::ln_p(a, b, c, midp, &f);
  }
  ln_p[v] = r;
  flags[v] = f;
}

}  // namespace

hipError_t launch_hwe(const ldp_variant_rec* recs, const uint32_t* hom1, const uint32_t* het, const uint32_t* hom2, uint32_t n, int midp, double* ln_p, uint8_t* flags,
                      hipStream_t stream) {
  if (!n) {
    return hipSuccess;
  }
  if (!ln_p || !flags || (!recs && (!hom1 || !het || !hom2))) {
    return hipErrorInvalidValue;
  }
  const uint32_t grid = (n + kHweThreads - 1) / kHweThreads;  // n < 2^32: at most 2^24 blocks
  hipLaunchKernelGGL(hwe_kernel, dim3(grid), dim3(kHweThreads), 0, stream, recs, hom1, het, hom2, n, midp, ln_p, flags);
  return hipGetLastError();
}

}  // namespace ldp
