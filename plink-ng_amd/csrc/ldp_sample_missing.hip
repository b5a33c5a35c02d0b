// ldp_sample_missing.hip -- per-sample missing-call counts of rows of the resident 2-bit image: ldp_sample_missing_counts(), what a host's
// --mind decides from.  A read-only pass in the SAMPLE direction: every other pass over the image reduces along a row, this one reduces
// down the columns.  Missing is code 11 in either orientation of a row (the inversion swaps 00 and 10 only), so `w & (w >> 1) & 0x55555555`
// is one flag per sample of a code dword, sixteen at a time.  The flags of successive rows are added in bit-sliced vertical counters held in
// registers -- 2-bit fields for 3 rows, 4-bit fields for 15, 8-bit fields for 255 (the reference's VcountIncr1To4 / 4To8 / 8To32 on the
// CPU, plink2_data.cc:10846-10990) -- so a row costs ~3 VALU operations per 16 samples, not 16 adds.
//
// Grid = row slabs x column groups.  A block owns one 128-byte column group (512 samples: rows are whole 128-byte units, so every block's
// loads are whole cache lines) and one slab of rows; its 256 threads are 8 sixteen-byte units across x 32 row lanes, lane l taking the
// slab's rows l, l + 32, ...: at most kSmRowsPerLane = 255 of them, the most an 8-bit field holds, so no field overflows whatever the data.
// At the end of the slab the 32 lanes' fields are summed per sample in LDS (32-bit) and the non-zero sums of samples below founder_ct go to
// the caller's zeroed array with one 32-bit vector atomicAdd each.  The padding columns beyond founder_ct are coded 11 in every row; they are
// counted like any column and dropped at that last step, the only place that knows founder_ct.  Integer adds commute: the result does not
// depend on how blocks are scheduled.  Row offsets are 64-bit (row * pitch passes 2^32 bytes on every real image).
#include "ldp_device.h"

namespace ldp {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kSmThreads = 256;
constexpr int kSmUnits = 8;                           // 16-byte units of one column group: 128 bytes, 512 samples
constexpr int kSmLanes = kSmThreads / kSmUnits;       // row lanes of a block
constexpr uint32_t kSmRowsPerLane = 255;              // an 8-bit field's worth
constexpr uint32_t kSmSlabRowsMax = kSmLanes * kSmRowsPerLane;
constexpr int kSmSamples = kSmUnits * 64;

// rows [row0, row0 + n_rows) of the image at `codes`; slab_rows <= kSmSlabRowsMax.  counts: founder_ct entries, zeroed by the host
__global__ __launch_bounds__(kSmThreads) void sample_missing_kernel(const uint8_t* __restrict__ codes, uint64_t pitch, uint64_t row0, uint32_t n_rows,
                                                                      uint32_t slab_rows, uint32_t founder_ct, uint32_t* counts) {
  __shared__ uint32_t sums[kSmSamples];
  const uint32_t unit = threadIdx.x & (kSmUnits - 1);
  const uint32_t lane = threadIdx.x / kSmUnits;
  const uint64_t slab_first = static_cast<uint64_t>(blockIdx.x) * slab_rows;
  const uint32_t slab_n = static_cast<uint32_t>(min(static_cast<uint64_t>(slab_rows), n_rows - slab_first));
  const uint8_t* col = codes + static_cast<uint64_t>(blockIdx.y) * (kSmUnits * 16) + unit * 16;
  for (uint32_t k = threadIdx.x; k < kSmSamples; k += kSmThreads) {
    sums[k] = 0;
  }
  // per dword d of the unit: two words of 4-bit fields, four words of 8-bit fields (which sample a field counts: the scatter below)
  uint32_t acc8[4][4], acc4[4][2];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      acc8[d][f] = 0;
    }
    acc4[d][0] = 0;
    acc4[d][1] = 0;
  }
  // the lane's rows in groups of 15 (five triples): 15 loads in flight, rows past the slab's end read nothing and count nothing
  for (uint32_t r = lane; r < slab_n; r += 15 * kSmLanes) {
    u32x4 w[15];
#pragma unroll
    for (int j = 0; j < 15; ++j) {
      const uint32_t rr = r + j * kSmLanes;
      u32x4 z = {0u, 0u, 0u, 0u};
      if (rr < slab_n) {
        z = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(col + (row0 + slab_first + rr) * pitch));
      }
      w[j] = z;
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) {
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        uint32_t a2 = 0;  // 2-bit fields: three flags at most
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const uint32_t x = w[3 * t + j][d];
          a2 += x & (x >> 1) & 0x55555555u;
        }
        acc4[d][0] += a2 & 0x33333333u;  // 4-bit fields: five triples = 15 at most
        acc4[d][1] += (a2 >> 2) & 0x33333333u;
      }
    }
    // 8-bit fields: a lane passes here at most 17 times with at most 15 per field = 255
#pragma unroll
    for (int d = 0; d < 4; ++d) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        acc8[d][2 * h] += acc4[d][h] & 0x0f0f0f0fu;
        acc8[d][2 * h + 1] += (acc4[d][h] >> 4) & 0x0f0f0f0fu;
        acc4[d][h] = 0;
      }
    }
  }
  __syncthreads();
  // byte b of acc8[d][2 h + q] is the field of bit 8 b + 4 q + 2 h of dword d = sample 4 b + 2 q + h of its sixteen
#pragma unroll
  for (int d = 0; d < 4; ++d) {
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int h = f >> 1, q = f & 1;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const uint32_t c = (acc8[d][f] >> (8 * b)) & 0xffu;
        if (c) {
          atomicAdd(&sums[unit * 64 + d * 16 + 4 * b + 2 * q + h], c);
        }
      }
    }
  }
  __syncthreads();
  const uint64_t s0 = static_cast<uint64_t>(blockIdx.y) * kSmSamples;
  for (uint32_t k = threadIdx.x; k < kSmSamples; k += kSmThreads) {
    const uint32_t c = sums[k];
    if (c && (s0 + k < founder_ct)) {
      atomicAdd(counts + s0 + k, c);
    }
  }
}

}  // namespace

// counts[s] += missing calls of sample s over rows [row0, row0 + n_rows) of the image (pitch a multiple of 128 bytes, at least
// ceil(founder_ct / 512) * 128); counts is the caller's to zero.  slab_rows_opt: rows per slab (test hook; clamped to the 8-bit fields' limit), 0 = chosen here
hipError_t launch_sample_missing(const uint8_t* codes, uint64_t pitch, uint64_t row0, uint32_t n_rows, uint32_t founder_ct, uint32_t* counts, uint32_t slab_rows_opt,
                                 hipStream_t stream) {
  if (!n_rows || !founder_ct) {
    return hipSuccess;
  }
  const uint64_t col_groups = (static_cast<uint64_t>(founder_ct) + kSmSamples - 1) / kSmSamples;
  if ((pitch % (kSmUnits * 16)) || (col_groups * (kSmUnits * 16) > pitch) || (col_groups > 65535)) {
    return hipErrorInvalidValue;
  }
  // full slabs where the image is large; a small image is cut into shorter slabs (whole lanes' worth of rows) so that the device still has
  // a few thousand blocks
  constexpr uint64_t kTargetBlocks = 4096;
  uint64_t slab_rows = kSmSlabRowsMax;
  const uint64_t slabs_wanted = std::max<uint64_t>((kTargetBlocks + col_groups - 1) / col_groups, 1);
  if (slab_rows_opt) {
    slab_rows = std::min<uint64_t>(slab_rows_opt, kSmSlabRowsMax);
  } else if (static_cast<uint64_t>(n_rows) < slabs_wanted * kSmSlabRowsMax) {
    slab_rows = (n_rows + slabs_wanted - 1) / slabs_wanted;
    slab_rows = std::max<uint64_t>((slab_rows + kSmLanes - 1) / kSmLanes * kSmLanes, 4 * kSmLanes);
    slab_rows = std::min<uint64_t>(slab_rows, kSmSlabRowsMax);
  }
  const uint32_t slabs = static_cast<uint32_t>((n_rows + slab_rows - 1) / slab_rows);
  hipLaunchKernelGGL(sample_missing_kernel, dim3(slabs, static_cast<uint32_t>(col_groups)), dim3(kSmThreads), 0, stream, codes, pitch, row0, n_rows,
                     static_cast<uint32_t>(slab_rows), founder_ct, counts);
  return hipGetLastError();
}

}  // namespace ldp
