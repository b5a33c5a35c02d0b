// ldp_sample_het.hip -- per-sample het-call counts, missing-call counts and weighted missing-call sums of rows of the resident 2-bit image:
// ldp_sample_het_counts(), what a host's --het forms its observed and expected heterozygosity from.  The second pass
// in the SAMPLE direction, laid out as sample_missing_kernel is (ldp_sample_missing.hip): grid = row slabs x 128-byte column groups, 256
// threads = 8 sixteen-byte units across x 32 row lanes, lane l taking the slab's rows l, l + 32, ...; 15 nontemporal 16-byte loads in flight
// per thread; 64-bit row offsets.  Per code dword w two flag words: het = w & ~(w >> 1) & 0x55555555 (code 01) and missing =
// w & (w >> 1) & 0x55555555 (code 11), both the same in either orientation of a row (the inversion swaps 00 and 10 only).
//
//   het_ct[s], missing_ct[s]: each flag word feeds its own set of the bit-sliced vertical counters (2-bit fields for 3 rows, 4-bit for 15,
//     8-bit for 255: a lane has at most kShRowsPerLane = 255 rows, so no field overflows whatever the data), merged per sample in LDS and added
//     to the caller's zeroed arrays with 32-bit atomics.  The padding columns beyond founder_ct (coded 11 in every row) are counted like any
//     column and dropped at that last step.
//   missing_weight[s] (kWeighted): sum of weight[row] over the rows where s is missing, modulo 2^64.  Missing calls are sparse, so the set
//     bits of the missing flags are taken one by one, each a 64-bit LDS add into the column group's 512-entry table; the table's non-zero
//     entries go out with 64-bit global atomics at the slab's end.  The padding columns are masked out of the flags BEFORE this walk (the
//     last column group would otherwise walk up to 511 set bits on every row).
//
// A row with include[row] == 0 is loaded and then zeroed: code 00 everywhere is neither het nor missing, so it contributes to nothing (and the
// loads stay independent of the include bytes).  include and weight are indexed by row of the launch (0 = row0).  A block takes its slab in
// passes of 480 rows (15 per lane); the pass's include bytes and weights are read once by the block into LDS, behind the row loads, and a
// lane picks its own rows' entries from there.  Integer adds commute: no result depends on how blocks are scheduled or on the slab length.
#include "ldp_device.h"

namespace ldp {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kShThreads = 256;
constexpr int kShUnits = 8;                           // 16-byte units of one column group: 128 bytes, 512 samples
constexpr int kShLanes = kShThreads / kShUnits;       // row lanes of a block
constexpr uint32_t kShRowsPerLane = 255;              // an 8-bit field's worth
constexpr uint32_t kShSlabRowsMax = kShLanes * kShRowsPerLane;
constexpr int kShSamples = kShUnits * 64;
constexpr int kShDepth = 15;                          // loads in flight per thread (five triples)
constexpr uint32_t kShPassRows = kShDepth * kShLanes;  // rows a block takes per pass

// one set of vertical counters of a thread: per dword d of the unit two words of 4-bit fields, four words of 8-bit fields
struct VCount {
  uint32_t acc8[4][4], acc4[4][2];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        acc8[d][f] = 0;
      }
      acc4[d][0] = 0;
      acc4[d][1] = 0;
    }
  }
  // a2: 2-bit fields holding the flags of three rows
  __device__ __forceinline__ void add_triple(int d, uint32_t a2) {
    acc4[d][0] += a2 & 0x33333333u;  // 4-bit fields: five triples = 15 at most
    acc4[d][1] += (a2 >> 2) & 0x33333333u;
  }
  // 8-bit fields: a lane passes here at most 17 times with at most 15 per field = 255
  __device__ __forceinline__ void fold() {
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
  // byte b of acc8[d][2 h + q] is the field of bit 8 b + 4 q + 2 h of dword d = sample 4 b + 2 q + h of its sixteen
  __device__ __forceinline__ void scatter(uint32_t* sums, uint32_t unit) const {
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
  }
};

// rows [row0, row0 + n_rows) of the image at `codes`; slab_rows <= kShSlabRowsMax.  include (NULL: every row) and weight: n_rows entries;
// het_ct / missing_ct / missing_weight: founder_ct entries, zeroed by the host
template <bool kWeighted>
__global__ __launch_bounds__(kShThreads) void sample_het_kernel(const uint8_t* __restrict__ codes, uint64_t pitch, uint64_t row0, uint32_t n_rows, uint32_t slab_rows,
                                                                uint32_t founder_ct, const uint8_t* __restrict__ include, const uint64_t* __restrict__ weight,
                                                                uint32_t* het_ct, uint32_t* missing_ct, unsigned long long* missing_weight) {
  __shared__ uint32_t sums_het[kShSamples];
  __shared__ uint32_t sums_mis[kShSamples];
  __shared__ unsigned long long sums_w[kWeighted ? kShSamples : 1];
  __shared__ unsigned long long row_w[kWeighted ? kShPassRows : 1];  // the current pass's rows: weight[], include[]
  __shared__ uint8_t row_inc[kShPassRows];
  const uint32_t unit = threadIdx.x & (kShUnits - 1);
  const uint32_t lane = threadIdx.x / kShUnits;
  const uint64_t slab_first = static_cast<uint64_t>(blockIdx.x) * slab_rows;
  const uint32_t slab_n = static_cast<uint32_t>(min(static_cast<uint64_t>(slab_rows), n_rows - slab_first));
  const uint8_t* col = codes + static_cast<uint64_t>(blockIdx.y) * (kShUnits * 16) + unit * 16;
  const uint64_t s0 = static_cast<uint64_t>(blockIdx.y) * kShSamples;
  for (uint32_t k = threadIdx.x; k < kShSamples; k += kShThreads) {
    sums_het[k] = 0;
    sums_mis[k] = 0;
    if constexpr (kWeighted) {
      sums_w[k] = 0;
    }
  }
  // the flag bits of dword d that belong to samples below founder_ct (the weighted walk only)
  uint32_t real[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const uint64_t first = s0 + unit * 64 + d * 16;
    const uint32_t v = (first >= founder_ct) ? 0u : static_cast<uint32_t>(min(static_cast<uint64_t>(16), founder_ct - first));
    real[d] = (v == 16) ? 0x55555555u : (((1u << (2 * v)) - 1u) & 0x55555555u);
  }
  unsigned long long* const my_w = sums_w + (kWeighted ? unit * 64 : 0);  // the unit's 64 entries of the table
  VCount het, mis;
  het.clear();
  mis.clear();
  if constexpr (kWeighted) {
    __syncthreads();  // the table is zero before anyone adds to it
  }
  // the lane's rows in groups of 15 (five triples): 15 loads in flight, rows past the slab's end read nothing and count nothing
  // (the trip count is the block's, not the lane's: the per-row arguments are staged by all threads between two barriers)
  for (uint32_t base = 0; base < slab_n; base += kShPassRows) {
    const uint32_t r = base + lane;
    u32x4 w[kShDepth];
#pragma unroll
    for (int j = 0; j < kShDepth; ++j) {
      const uint32_t rr = r + j * kShLanes;
      u32x4 z = {0u, 0u, 0u, 0u};
      if (rr < slab_n) {
        z = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(col + (row0 + slab_first + rr) * pitch));
      }
      w[j] = z;
    }
    // the pass's 480 rows' include bytes and weights: read once per block (every row's entry is wanted by the eight units of its lane), not once
    // per thread -- thirty more vector loads per thread cost more than the walk itself
    if (include || kWeighted) {
      for (uint32_t k = threadIdx.x; k < kShPassRows; k += kShThreads) {
        const uint32_t rr = base + k;
        uint8_t inc = 0;
        if (rr < slab_n) {
          inc = include ? include[slab_first + rr] : 1;
        }
        row_inc[k] = inc;
        if constexpr (kWeighted) {
          row_w[k] = (rr < slab_n) ? weight[slab_first + rr] : 0;
        }
      }
      __syncthreads();
      if (include) {
#pragma unroll
        for (int j = 0; j < kShDepth; ++j) {
          w[j] &= row_inc[lane + j * kShLanes] ? 0xffffffffu : 0u;
        }
      }
    }
    if constexpr (kWeighted) {
      // the weighted walk, one loop per row: the four dwords' missing flags (even bits) interleave into one 64-bit word -- bit 32 h + 2 i + q is
      // sample i of dword 2 h + q --, so a wave pays for the most missing calls any of its lanes has among 64 samples, not four times among 16
#pragma unroll
      for (int j = 0; j < kShDepth; ++j) {
        uint32_t m[4];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const uint32_t x = w[j][d];
          m[d] = x & (x >> 1) & real[d];
        }
        unsigned long long walk = static_cast<unsigned long long>(m[0] | (m[1] << 1)) | (static_cast<unsigned long long>(m[2] | (m[3] << 1)) << 32);
        if (walk) {
          const unsigned long long wt = row_w[lane + j * kShLanes];
          do {
            const uint32_t bit = static_cast<uint32_t>(__builtin_ctzll(walk));
            walk &= walk - 1;
            atomicAdd(&my_w[(((bit >> 5) * 2 + (bit & 1)) << 4) + ((bit & 31) >> 1)], wt);
          } while (walk);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) {
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        uint32_t h2 = 0, m2 = 0;  // 2-bit fields: three flags at most
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const uint32_t x = w[3 * t + j][d];
          const uint32_t hi = x >> 1;
          h2 += x & ~hi & 0x55555555u;
          m2 += x & hi & 0x55555555u;
        }
        het.add_triple(d, h2);
        mis.add_triple(d, m2);
      }
    }
    het.fold();
    mis.fold();
    if (include || kWeighted) {
      __syncthreads();  // everybody has read the pass's entries before the next pass overwrites them
    }
  }
  __syncthreads();
  het.scatter(sums_het, unit);
  mis.scatter(sums_mis, unit);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < kShSamples; k += kShThreads) {
    if (s0 + k < founder_ct) {
      const uint32_t h = sums_het[k], m = sums_mis[k];
      if (h) {
        atomicAdd(het_ct + s0 + k, h);
      }
      if (m) {
        atomicAdd(missing_ct + s0 + k, m);
      }
      if constexpr (kWeighted) {
        const unsigned long long ws = sums_w[k];
        if (ws) {
          atomicAdd(missing_weight + s0 + k, ws);
        }
      }
    }
  }
}

}  // namespace

// het_ct[s] += het calls, missing_ct[s] += missing calls and (weight != NULL) missing_weight[s] += the weights of the missing calls of sample
// s over the included rows of [row0, row0 + n_rows) of the image (pitch a multiple of 128 bytes, at least ceil(founder_ct / 512) * 128); the
// three arrays are the caller's to zero.  include / weight: device arrays of n_rows entries (include NULL: every row).  slab_rows_opt: rows per
// slab (test hook; clamped to the 8-bit fields' limit), 0 = chosen here
hipError_t launch_sample_het(const uint8_t* codes, uint64_t pitch, uint64_t row0, uint32_t n_rows, uint32_t founder_ct, const uint8_t* include, const uint64_t* weight,
                             uint32_t* het_ct, uint32_t* missing_ct, uint64_t* missing_weight, uint32_t slab_rows_opt, hipStream_t stream) {
  if (!n_rows || !founder_ct) {
    return hipSuccess;
  }
  const uint64_t col_groups = (static_cast<uint64_t>(founder_ct) + kShSamples - 1) / kShSamples;
  if ((pitch % (kShUnits * 16)) || (col_groups * (kShUnits * 16) > pitch) || (col_groups > 65535) || (weight && !missing_weight)) {
    return hipErrorInvalidValue;
  }
  // slabs as launch_sample_missing cuts them: full ones where the image is large, shorter ones (whole lanes' worth of rows) on a small image
  constexpr uint64_t kTargetBlocks = 4096;
  uint64_t slab_rows = kShSlabRowsMax;
  const uint64_t slabs_wanted = std::max<uint64_t>((kTargetBlocks + col_groups - 1) / col_groups, 1);
  if (slab_rows_opt) {
    slab_rows = std::min<uint64_t>(slab_rows_opt, kShSlabRowsMax);
  } else if (static_cast<uint64_t>(n_rows) < slabs_wanted * kShSlabRowsMax) {
    slab_rows = (n_rows + slabs_wanted - 1) / slabs_wanted;
    slab_rows = std::max<uint64_t>((slab_rows + kShLanes - 1) / kShLanes * kShLanes, 4 * kShLanes);
    slab_rows = std::min<uint64_t>(slab_rows, kShSlabRowsMax);
  }
  const uint32_t slabs = static_cast<uint32_t>((n_rows + slab_rows - 1) / slab_rows);
  const dim3 grid(slabs, static_cast<uint32_t>(col_groups));
  if (weight) {
    hipLaunchKernelGGL(sample_het_kernel<true>, grid, dim3(kShThreads), 0, stream, codes, pitch, row0, n_rows, static_cast<uint32_t>(slab_rows), founder_ct, include, weight,
                       het_ct, missing_ct, reinterpret_cast<unsigned long long*>(missing_weight));
  } else {
    hipLaunchKernelGGL(sample_het_kernel<false>, grid, dim3(kShThreads), 0, stream, codes, pitch, row0, n_rows, static_cast<uint32_t>(slab_rows), founder_ct, include, weight,
                       het_ct, missing_ct, static_cast<unsigned long long*>(nullptr));
  }
  return hipGetLastError();
}

}  // namespace ldp
