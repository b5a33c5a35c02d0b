// ldp_hwe_host.cpp -- ldp_hwe_ln_p_host(): the exact Hardy-Weinberg test of one variant on the host, the arithmetic of hwe_kernel
// (ldp_hwe_core.h) compiled for the CPU.  What a front-end uses where the counts come from its own pass over the rows, and what device
// results at sample counts beyond an exact evaluation's reach are compared against.  No device, no engine, no state: any thread may call it.
#include <limits>

#include "../../include/ldprune_hip.h"
#include "ldp_hwe_core.h"

extern "C" double ldp_hwe_ln_p_host(uint32_t hom1, uint32_t het, uint32_t hom2, int midp, uint8_t* flags) {
  if (static_cast<uint64_t>(hom1) + het + hom2 >= (1ull << 31)) {
    if (flags) {
      *flags = 0x80;
    }
    return std::numeric_limits<double>::quiet_NaN();
  }
  return ldp_hwe::ln_p(hom1, het, hom2, midp, flags);
}
