// ldp_compact.hip -- rows of the resident image (and of the per-row arrays beside it) move to the indices a restricted engine gives
// them: ldp_restrict_variants().  A pure copy: 16-byte loads and stores (every row pitch here is a multiple of 16 bytes: image rows
// of 128, records of 32, checkpoint slots of 16), the source row of each destination row read from a device array, no LDS, no
// atomics.  Which rows may move in one launch without a row being overwritten before it is read is the host's business
// (ldp_compact_schedule.h); a launch only requires that ITS source and destination rows do not overlap.
#include "ldp_device.h"

namespace ldp {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kCompactThreads = 256;
constexpr int kCompactUnroll = 4;

// destination row dst_row0 + r <- source row (src_idx ? src_idx[r] : r), r < n_rows; a row = units_per_row 16-byte units.  One flat
// grid over (row, unit), n_rows * units_per_row < 2^32: a thread moves kCompactUnroll units a block width apart -- the source indices of
// all of them first, then every load, then the stores.  A thread past the end repeats the last unit's loads (no branch between the
// loads: they stay in flight together) and stores nothing.
__global__ __launch_bounds__(kCompactThreads) void compact_rows_kernel(u32x4* dst, const u32x4* src, uint32_t units_per_row, const uint32_t* __restrict__ src_idx,
                                                                         uint64_t dst_row0, uint32_t total) {
  const uint32_t base = blockIdx.x * (kCompactThreads * kCompactUnroll) + threadIdx.x;
  uint32_t r[kCompactUnroll], u[kCompactUnroll], from[kCompactUnroll];
  u32x4 held[kCompactUnroll];
#pragma unroll
  for (int j = 0; j < kCompactUnroll; ++j) {
    const uint32_t idx = min(base + j * kCompactThreads, total - 1);
    r[j] = idx / units_per_row;
    u[j] = idx - r[j] * units_per_row;
  }
#pragma unroll
  for (int j = 0; j < kCompactUnroll; ++j) {
    from[j] = src_idx ? src_idx[r[j]] : r[j];
  }
#pragma unroll
  for (int j = 0; j < kCompactUnroll; ++j) {
    held[j] = __builtin_nontemporal_load(src + static_cast<uint64_t>(from[j]) * units_per_row + u[j]);
  }
#pragma unroll
  for (int j = 0; j < kCompactUnroll; ++j) {
    if (base + j * kCompactThreads < total) {
      __builtin_nontemporal_store(held[j], dst + (dst_row0 + r[j]) * units_per_row + u[j]);
    }
  }
}

// the one-byte row flags (d_stored_inv), out of place: dst[k] = src[src_idx[k]]
__global__ __launch_bounds__(256) void gather_bytes_kernel(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, const uint32_t* __restrict__ src_idx, uint32_t n) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k < n) {
    dst[k] = src[src_idx[k]];
  }
}

}  // namespace

hipError_t launch_compact_rows(void* dst, const void* src, uint64_t row_bytes, const uint32_t* src_idx, uint64_t dst_row0, uint32_t n_rows, hipStream_t stream) {
  if (!n_rows) {
    return hipSuccess;
  }
  const uint64_t total = static_cast<uint64_t>(n_rows) * (row_bytes / 16);
  // (one launch indexes its units with 32 bits, a block's last thread included: the caller cuts larger jobs into batches)
  if ((row_bytes & 15) || (!row_bytes) || (total > 0xffffffffull - kCompactThreads * kCompactUnroll)) {
    return hipErrorInvalidValue;
  }
  const uint32_t blocks = static_cast<uint32_t>((total + kCompactThreads * kCompactUnroll - 1) / (kCompactThreads * kCompactUnroll));
  hipLaunchKernelGGL(compact_rows_kernel, dim3(blocks), dim3(kCompactThreads), 0, stream, static_cast<u32x4*>(dst), static_cast<const u32x4*>(src),
                     static_cast<uint32_t>(row_bytes / 16), src_idx, dst_row0, static_cast<uint32_t>(total));
  return hipGetLastError();
}

hipError_t launch_gather_bytes(uint8_t* dst, const uint8_t* src, const uint32_t* src_idx, uint32_t n, hipStream_t stream) {
  if (!n) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(gather_bytes_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, dst, src, src_idx, n);
  return hipGetLastError();
}

}  // namespace ldp
