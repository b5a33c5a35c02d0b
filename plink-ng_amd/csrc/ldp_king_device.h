// ldp_king_device.h -- what ldp_king.hip (the kernels) and ldp_engine_king.cpp (the host side of ldp_king_counts_block / ldp_king_block_hits)
// share: the slab and scratch constants and the launch wrappers.  A header of its own: nothing else includes it.
#ifndef LDP_KING_DEVICE_H
#define LDP_KING_DEVICE_H

#include "ldp_device.h"

namespace ldp {

// ldp_king.hip: KING-robust counts of sample pairs, slab by slab.  A slab is slab_variants image rows (a multiple of kKingSlabMin, at most
// kKingSlabMax: the f32 accumulators stay far below 2^24); king_slab_variants() picks the longest slab whose two strip sets (row samples and
// column samples, slab_variants / 4 bytes per sample) stay below kKingScratchCap.
constexpr uint32_t kKingSlabMin = 256;
constexpr uint32_t kKingSlabMax = 65536;
constexpr uint64_t kKingScratchCap = 128ull << 20;
constexpr uint32_t kKingStripSamples = 256;  // strips are written for whole groups of this many samples, from a multiple of it on
uint32_t king_slab_variants(uint32_t row_ct, uint32_t col_ct);
// strips[(s - s_base) * (slab_variants / 4) ...], s in [s_base, s_base + 256 sample_blocks): the 2-bit codes of sample s at image rows [row0, row0 + n_rows),
// code 11 for the rest of the slab, for rows with include[row - row0] == 0 (include NULL: none) and for s >= founder_ct
hipError_t launch_king_transpose(const uint8_t* codes, uint64_t pitch, uint64_t row0, uint32_t n_rows, const uint8_t* include, uint32_t founder_ct, uint32_t s_base,
                                 uint32_t sample_blocks, uint8_t* strips, uint32_t slab_variants, hipStream_t stream);
// counts (ldp_king_counts_t[row_ct][ld]) += the slab's five integers of the pairs col < row of rows [row_first, +row_ct) x columns [col_first, +col_ct)
hipError_t launch_king_pairs(const uint8_t* strips_a, const uint8_t* strips_b, uint32_t slab_variants, uint32_t a_base, uint32_t b_base, uint32_t row_first, uint32_t row_ct,
                             uint32_t col_first, uint32_t col_ct, void* counts, uint64_t ld, hipStream_t stream);
// hits (ldp_king_hit[capacity]) <- the pairs col < row with !(kinship < min_kinship); *count (device, zeroed by the caller) += their number
hipError_t launch_king_hits(const void* counts, uint64_t ld, uint32_t row_first, uint32_t row_ct, uint32_t col_first, uint32_t col_ct, double min_kinship, void* hits,
                            uint64_t capacity, uint64_t* count, hipStream_t stream);

}  // namespace ldp
#endif
