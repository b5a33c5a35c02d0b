// ldp_king.hip -- KING-robust kinship counts of SAMPLE pairs from the resident 2-bit image: ldp_king_counts_block() / ldp_king_block_hits(),
// what a host's --make-king-table prints.  Per sample three indicator vectors over the variants -- t = het, h = hom,
// x = +1 hom-REF / -1 hom-ALT, all 0 at a missing call -- and per pair five products: t.t (hethet), t_row.h_col, h_row.t_col, h.h (homhom) and
// x.x, with ibs0 = (h.h - x.x) / 2.  The image is variant-major and the products run over the variants, so the work is done slab by slab:
//
//   king_transpose_kernel: a slab of K image rows x a range of samples -> sample-major strips of K / 4 bytes each (the image's own 2-bit
//     codes, variant k of the slab at bits 2 (k & 15) of dword k / 16).  Rows whose include byte is 0, rows beyond the range and samples
//     beyond founder_ct are written as code 11 (missing): t = h = x = 0 there, so they drop out of every product by themselves.
//   king_pair_kernel: 64 x 64 sample tiles on the absolute sample grid (rows = later samples, columns = earlier ones), four waves, one 32 x 32
//     block each; a block without a wanted pair (column < row, both inside the request) does nothing.  A lane (r = lane & 31, half = lane >> 5)
//     loads 16 bytes of the strips of row sample r and of column sample r per two k-steps: 64 variants, expanded to the three E2M1 operands
//     with one v_bitop3 per 8 values each, and five v_mfma_scale_f32_32x32x64_f8f6f4 per k-step (E8M0 scale 1/2: +-2.0 -> +-1).  Both operands
//     of a product take the same variants in the same order, which is all a dot product asks of the K order.  The f32 accumulators hold
//     integers of at most K <= kKingSlabMax < 2^24: exact.  At the slab's end they are converted and added to the block's uint32 results (a
//     pair belongs to one lane of one wave of the launch and launches are ordered by the stream: plain read-modify-write).
//   king_hits_kernel: kinship per pair in FP64 (ComputeKinship, plink2_matrix_calc.cc) with __ddiv_rn -- every integer involved is below
//     2^53, so the double is the host's bit for bit -- and the pairs with !(kinship < min_kinship) appended through one atomic counter.
//
// All five integers are unchanged when a variant's 00 and 10 are swapped: rows the count pass stored inverted need no un-flipping.
#include "ldp_king_device.h"
#include "ldp_mfma_device.h"

namespace ldp {

namespace {

constexpr int kKtThreads = 256;
constexpr uint32_t kKtSamples = 256;   // a transpose block: 256 samples (16 image dwords) x 256 variants (16 strip dwords)
constexpr uint32_t kKtVariants = 256;
constexpr int kKpThreads = 256;
constexpr uint32_t kKpTile = 64;       // samples per tile side: 2 x 2 blocks of 32

// het indicator of the odd samples' nibbles: 2.0 at nibble bit 2 where b0 & !b1 (fp4_x / fp4_n have the idiom)
__device__ __forceinline__ uint32_t fp4_t(uint32_t X) { return __builtin_amdgcn_bitop3_b32(X, X >> 1, 0x44444444u, 0x20); }  // a & !b & c
// hom indicator |x|: 2.0 where !b0
__device__ __forceinline__ uint32_t fp4_h(uint32_t X) { return ~X & 0x44444444u; }

__device__ __forceinline__ void king_operands(uint32_t c0, uint32_t c1, Frag& x, Frag& h, Frag& t) {
  const uint32_t c[4] = {c0, c0 << 2, c1, c1 << 2};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    x.d[d] = fp4_x(c[d]);
    h.d[d] = fp4_h(c[d]);
    t.d[d] = fp4_t(c[d]);
  }
}

// strips[(s - s_base) * strip_bytes + k / 4] for samples [s_base, s_base + 256 gridDim.y) and variants k of the slab: image rows
// [row0, row0 + n_rows) are the slab's first n_rows variants (n_rows <= strip_bytes * 4, a multiple of 256); include: n_rows bytes or NULL
__global__ __launch_bounds__(kKtThreads) void king_transpose_kernel(const uint8_t* __restrict__ codes, uint64_t pitch, uint64_t row0, uint32_t n_rows,
                                                                    const uint8_t* __restrict__ include, uint32_t founder_ct, uint32_t s_base, uint8_t* __restrict__ strips,
                                                                    uint64_t strip_bytes) {
  __shared__ uint32_t tile[kKtSamples][17];
  const uint32_t sg = threadIdx.x & 15, kg = threadIdx.x >> 4;
  const uint32_t k0 = blockIdx.x * kKtVariants + kg * 16;
  const uint64_t s0 = static_cast<uint64_t>(s_base) + static_cast<uint64_t>(blockIdx.y) * kKtSamples + sg * 16;  // the dword's first sample
  const bool in_row = (s0 / 4 + 4 <= pitch);
  // samples at or beyond founder_ct: forced to 11
  uint32_t pad = 0;
  if (s0 >= founder_ct) {
    pad = 0xffffffffu;
  } else if (founder_ct - s0 < 16) {
    pad = 0xffffffffu << (2 * static_cast<uint32_t>(founder_ct - s0));
  }
  uint32_t w[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t k = k0 + j;
    uint32_t v = 0xffffffffu;
    if (in_row && (k < n_rows) && (pad != 0xffffffffu) && (!include || include[k])) {
      v = *reinterpret_cast<const uint32_t*>(codes + (row0 + k) * pitch + s0 / 4);
    }
    w[j] = v | pad;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      o |= ((w[j] >> (2 * i)) & 3u) << (2 * j);
    }
    tile[sg * 16 + i][kg] = o;
  }
  __syncthreads();
  // thread = sample: its 64 bytes of this block's 256 variants
  uint32_t* dst = reinterpret_cast<uint32_t*>(strips + (static_cast<uint64_t>(blockIdx.y) * kKtSamples + threadIdx.x) * strip_bytes + blockIdx.x * (kKtVariants / 4));
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    mf_u4 o = {tile[threadIdx.x][4 * q], tile[threadIdx.x][4 * q + 1], tile[threadIdx.x][4 * q + 2], tile[threadIdx.x][4 * q + 3]};
    *reinterpret_cast<mf_u4*>(dst + 4 * q) = o;
  }
}

struct KingCounts {
  uint32_t hethet, het_row_hom_col, hom_row_het_col, homhom, ibs0;
};

// out[(row - row_first) * ld + (col - col_first)] += the slab's counts, for the pairs col < row of the request.  strips_a / strips_b: the
// strips of the samples from a_base / b_base on (multiples of 64, at most row_first / col_first), k_pairs * 128 variants each
__global__ __launch_bounds__(kKpThreads) void king_pair_kernel(const uint8_t* __restrict__ strips_a, const uint8_t* __restrict__ strips_b, uint64_t strip_bytes, uint32_t k_pairs,
                                                               uint32_t a_base, uint32_t b_base, uint32_t row_first, uint32_t row_end, uint32_t col_first, uint32_t col_end,
                                                               KingCounts* out, uint64_t ld) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t r0 = a_base + blockIdx.y * kKpTile + (wave >> 1) * kMfBlock;
  const uint32_t c0 = b_base + blockIdx.x * kKpTile + (wave & 1) * kMfBlock;
  // the block's wanted pairs: rows [r_lo, r_hi], columns [c_lo, c_hi], column < row
  const uint32_t r_lo = max(r0, row_first), c_lo = max(c0, col_first);
  const uint32_t r_hi_x = min(r0 + kMfBlock, row_end), c_hi_x = min(c0 + kMfBlock, col_end);  // exclusive
  if ((r_lo >= r_hi_x) || (c_lo >= c_hi_x) || (c_lo + 1 >= r_hi_x)) {
    return;  // (wave-uniform; no barrier in this kernel)
  }
  const uint32_t r = lane & 31, half = lane >> 5;
  const uint8_t* pa = strips_a + static_cast<uint64_t>(r0 - a_base + r) * strip_bytes + half * 16;
  const uint8_t* pb = strips_b + static_cast<uint64_t>(c0 - b_base + r) * strip_bytes + half * 16;
  mf_v16f acc_tt, acc_th, acc_ht, acc_hh, acc_xx;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    acc_tt[i] = 0.f;
    acc_th[i] = 0.f;
    acc_ht[i] = 0.f;
    acc_hh[i] = 0.f;
    acc_xx[i] = 0.f;
  }
  mf_u4 a = *reinterpret_cast<const mf_u4*>(pa);
  mf_u4 b = *reinterpret_cast<const mf_u4*>(pb);
  for (uint32_t q = 0; q < k_pairs; ++q) {
    const mf_u4 ca = a, cb = b;
    if (q + 1 < k_pairs) {  // the next two k-steps' codes, in flight behind this pair's products
      a = *reinterpret_cast<const mf_u4*>(pa + static_cast<uint64_t>(q + 1) * 32);
      b = *reinterpret_cast<const mf_u4*>(pb + static_cast<uint64_t>(q + 1) * 32);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      Frag xa, ha, ta, xb, hb, tb;
      king_operands(ca[2 * s], ca[2 * s + 1], xa, ha, ta);
      king_operands(cb[2 * s], cb[2 * s + 1], xb, hb, tb);
      acc_tt = mfma_fp4(ta, tb, acc_tt);
      acc_th = mfma_fp4(ta, hb, acc_th);
      acc_ht = mfma_fp4(ha, tb, acc_ht);
      acc_hh = mfma_fp4(ha, hb, acc_hh);
      acc_xx = mfma_fp4(xa, xb, acc_xx);
    }
  }
  // C[row of a][column of b]: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const uint32_t col = c0 + r;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t row = r0 + (i & 3) + 8 * (i >> 2) + 4 * half;
    if ((row >= row_first) && (row < row_end) && (col >= col_first) && (col < col_end) && (col < row)) {
      KingCounts* p = out + static_cast<uint64_t>(row - row_first) * ld + (col - col_first);
      const int32_t hh = static_cast<int32_t>(acc_hh[i]), xx = static_cast<int32_t>(acc_xx[i]);
      p->hethet += static_cast<uint32_t>(static_cast<int32_t>(acc_tt[i]));
      p->het_row_hom_col += static_cast<uint32_t>(static_cast<int32_t>(acc_th[i]));
      p->hom_row_het_col += static_cast<uint32_t>(static_cast<int32_t>(acc_ht[i]));
      p->homhom += static_cast<uint32_t>(hh);
      p->ibs0 += static_cast<uint32_t>((hh - xx) >> 1);  // every variant adds 0 or 2 to hh - xx
    }
  }
}

struct KingHit {
  uint32_t row, col;
  KingCounts c;
};

// kinship = 0.5 - (4 ibs0 + het_row_hom_col + hom_row_het_col) / (4 (hethet + min(het_row_hom_col, hom_row_het_col))): 0 / 0 is NaN (kept by
// !(kinship < min)), a positive numerator over 0 gives -inf (dropped)
__global__ __launch_bounds__(256) void king_hits_kernel(const KingCounts* __restrict__ counts, uint64_t ld, uint32_t row_first, uint32_t row_ct, uint32_t col_first,
                                                        uint32_t col_ct, double min_kinship, KingHit* hits, unsigned long long capacity, unsigned long long* count) {
  const uint32_t cj = blockIdx.x * blockDim.x + threadIdx.x;
  if (cj >= col_ct) {
    return;
  }
  for (uint32_t ri = blockIdx.y; ri < row_ct; ri += gridDim.y) {
    if (col_first + cj >= row_first + ri) {
      continue;
    }
    const KingCounts c = counts[static_cast<uint64_t>(ri) * ld + cj];
    const uint64_t num = 4ull * c.ibs0 + c.het_row_hom_col + c.hom_row_het_col;
    const uint64_t den = 4ull * (static_cast<uint64_t>(c.hethet) + min(c.het_row_hom_col, c.hom_row_het_col));
    const double kinship = 0.5 - __ddiv_rn(static_cast<double>(num), static_cast<double>(den));
    if (!(kinship < min_kinship)) {
      const unsigned long long slot = atomicAdd(count, 1ull);
      if (slot < capacity) {
        KingHit hit;
        hit.row = row_first + ri;
        hit.col = col_first + cj;
        hit.c = c;
        hits[slot] = hit;
      }
    }
  }
}

}  // namespace

uint32_t king_slab_variants(uint32_t row_ct, uint32_t col_ct) {
  // both strip sets, each padded to whole transpose blocks and one more for the alignment of its base
  const uint64_t samples = (static_cast<uint64_t>(row_ct) + 2 * kKtSamples) + (static_cast<uint64_t>(col_ct) + 2 * kKtSamples);
  uint64_t k = kKingScratchCap * 4 / samples;
  k = k / kKingSlabMin * kKingSlabMin;
  return static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(k, kKingSlabMin), kKingSlabMax));
}

hipError_t launch_king_transpose(const uint8_t* codes, uint64_t pitch, uint64_t row0, uint32_t n_rows, const uint8_t* include, uint32_t founder_ct, uint32_t s_base,
                                 uint32_t sample_blocks, uint8_t* strips, uint32_t slab_variants, hipStream_t stream) {
  if (!sample_blocks || (slab_variants % kKingSlabMin) || !slab_variants || (n_rows > slab_variants) || (s_base % kKtSamples) || (pitch % 4) || (sample_blocks > 65535)) {
    return hipErrorInvalidValue;
  }
  const dim3 grid(slab_variants / kKtVariants, sample_blocks);
  hipLaunchKernelGGL(king_transpose_kernel, grid, dim3(kKtThreads), 0, stream, codes, pitch, row0, n_rows, include, founder_ct, s_base, strips,
                     static_cast<uint64_t>(slab_variants / 4));
  return hipGetLastError();
}

hipError_t launch_king_pairs(const uint8_t* strips_a, const uint8_t* strips_b, uint32_t slab_variants, uint32_t a_base, uint32_t b_base, uint32_t row_first, uint32_t row_ct,
                             uint32_t col_first, uint32_t col_ct, void* counts, uint64_t ld, hipStream_t stream) {
  if (!row_ct || !col_ct) {
    return hipSuccess;
  }
  if ((slab_variants % 128) || (a_base % kKpTile) || (b_base % kKpTile) || (a_base > row_first) || (b_base > col_first)) {
    return hipErrorInvalidValue;
  }
  const uint32_t row_end = row_first + row_ct, col_end = col_first + col_ct;
  const dim3 grid((col_end - b_base + kKpTile - 1) / kKpTile, (row_end - a_base + kKpTile - 1) / kKpTile);
  if (grid.y > 65535) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(king_pair_kernel, grid, dim3(kKpThreads), 0, stream, strips_a, strips_b, static_cast<uint64_t>(slab_variants / 4), slab_variants / 128, a_base, b_base,
                     row_first, row_end, col_first, col_end, static_cast<KingCounts*>(counts), ld);
  return hipGetLastError();
}

hipError_t launch_king_hits(const void* counts, uint64_t ld, uint32_t row_first, uint32_t row_ct, uint32_t col_first, uint32_t col_ct, double min_kinship, void* hits,
                            uint64_t capacity, uint64_t* count, hipStream_t stream) {
  if (!row_ct || !col_ct) {
    return hipSuccess;
  }
  const dim3 grid((col_ct + 255) / 256, std::min<uint32_t>(row_ct, 65535));
  hipLaunchKernelGGL(king_hits_kernel, grid, dim3(256), 0, stream, static_cast<const KingCounts*>(counts), ld, row_first, row_ct, col_first, col_ct, min_kinship,
                     static_cast<KingHit*>(hits), static_cast<unsigned long long>(capacity), reinterpret_cast<unsigned long long*>(count));
  return hipGetLastError();
}

}  // namespace ldp
