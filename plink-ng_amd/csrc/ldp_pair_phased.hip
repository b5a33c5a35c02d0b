// ldp_pair_phased.hip -- what --r2-phased / --r-phased need beyond the six integers of the pair kernels (gfx950 / CDNA4).
//
// The haplotype-frequency statistic of a pair (ComputeR2NondosagePhasedStats, plink2_ld.cc:6545-6588) wants, over the jointly called
// samples: their number, the two allele sums, the haplotypes KNOWN to carry both counted alleles and the samples heterozygous at
// both variants.  ldp_pair_stats_t holds the first three and sum g_i g_j (from nm, sum1, sum2, dot: x = 1 - g on called samples).
// Missing is ONE number,
//     H[j][i] = sum_s e_j(s) e_i(s),   e = (code == 01),
// a 0/1 matrix product over the same resident 2-bit image: missing calls and padding samples are coded 11 and add nothing, there
// is no bias term and no orientation (inverting a row swaps 00 and 10).  Then
//     unknown_hethet = H,    known_dotprod = (sum g_i g_j - H) / 2        (a double heterozygote adds 1 to sum g g and is unknown).
// Phase information is a second engine whose rows code a sample's phase at the variant as 00 (phased het, phaseinfo 0: x = +1),
// 10 (phased het, phaseinfo 1: x = -1) or 01 (anything else: x = 0).  On those rows the six integers give P_i = ssq = the phased
// hets of a variant and dot = SS = #same - #diff over the samples phased at both; H gives the samples phased at neither, so
//     PP = P_i + P_j - N + H,   #diff = (PP - SS) / 2,   known_dotprod += PP - #diff,   unknown_hethet -= PP
// (HardcallPhasedR2Refine, plink2_ld.cc:3238-3262).  One kernel serves both images.
//
// pair_hethet_kernel puts H on the matrix pipe like its neighbours (ldp_pair_mfma.hip): FP4 operands expanded from the staged
// codes -- e as 0.5 in the low half of a nibble, E8M0 block scale 2 on both operands, so every product is 0 or 1 --, 256-sample
// stages through the LDS-DMA ring (StageGeom<4>), f32 accumulators, which hold the counts exactly below 2^24 (the callers refuse
// engines above ldp_matrix_pipe_max_founders()).  Every pair's count is wanted: no checkpoints, no early termination.
// phased_combine_kernel turns the two engines' integers into ldp_phased_stats_t and, for the hit form, applies the bound that
// decides which pairs reach the host (include/ldprune_hip.h: ldp_r2_phased_band_hits).
#include "ldp_device.h"
#include "ldp_pair_device.h"
#include "ldp_mfma_device.h"

namespace ldp {

constexpr uint32_t kHhRowBlocks = 4;                        // J0, J1, V0, V1
constexpr uint32_t kHhInstr = kHhRowBlocks * 2;             // DMA instructions per stage (64 sixteen-byte slots each)
constexpr uint32_t kHhDmaPerWave = kHhInstr / kMfWaves;     // 2
constexpr uint32_t kHhStageDwords = kHhInstr * 256;         // 8 KiB
constexpr uint32_t kHhStages = 4;                           // ring depth: 32 KiB of LDS
static_assert(kHhInstr % kMfWaves == 0, "every wave issues the same number of DMA instructions per stage (the vmcnt arithmetic of the ring)");

// 16 samples of 2-bit codes -> e = (code == 01) as E2M1 0.5 (nibble 0001) for the even and the odd samples: b0 & !b1 at nibble bit 0
__device__ __forceinline__ void fp4_e_of_dword(uint32_t X, uint32_t* e_even, uint32_t* e_odd) {
  const uint32_t Xs = X >> 2;
  *e_even = __builtin_amdgcn_bitop3_b32(X, X >> 1, 0x11111111u, 0x20);   // a & !b & c
  *e_odd = __builtin_amdgcn_bitop3_b32(Xs, Xs >> 1, 0x11111111u, 0x20);
}
__device__ __forceinline__ void fp4_e_of_codes(uint32_t c0, uint32_t c1, Frag& f) {
  fp4_e_of_dword(c0, &f.d[0], &f.d[1]);
  fp4_e_of_dword(c1, &f.d[2], &f.d[3]);
}

__global__ __launch_bounds__(kMfWaves * 64, 2) void pair_hethet_kernel(HetHetArgs A) {
  using G = StageGeom<4>;
  __shared__ __attribute__((aligned(16))) uint32_t lds[kHhStages * kHhStageDwords];
  const HetHetItem it = A.items[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t lane = tid & 63;
  const uint32_t r = lane & 31;
  const uint32_t h = lane >> 5;
  const uint32_t q = wave >> 1;   // J block of this wave's product
  const uint32_t vk = wave & 1;   // V block
  const uint32_t jfirst = it.jv + kMfBlock * q;
  const uint32_t vfirst = it.vv + kMfBlock * vk;
  const uint32_t n_stages = (A.founder_ct + G::kStageSamples - 1) / G::kStageSamples;  // (rows are whole 512-sample chunks: a stage never leaves its row)

  // ---- DMA plan: row-block slots 0, 1 = J0, J1; 2, 3 = V0, V1.  Instruction T fills slots 64 T .. 64 T + 63 of a stage: rows
  // 16 (T & 1) .. + 15 of row-block T >> 1, four pieces each.  Rows beyond the image read its last row: their pairs are never stored.
  const uint8_t* src[kHhDmaPerWave];
#pragma unroll
  for (int t = 0; t < static_cast<int>(kHhDmaPerWave); ++t) {
    const uint32_t T = wave + kMfWaves * t;
    const uint32_t blk = T >> 1;
    const uint32_t first = (blk < 2) ? (it.jv + kMfBlock * blk) : (it.vv + kMfBlock * (blk - 2));
    const uint32_t L = T * 64 + lane;
    const uint32_t rr = (L >> 2) & 31;
    const uint32_t col = (L & 3) ^ G::swizzle(rr);
    uint32_t var = first + rr;
    var = (var < A.n_local) ? var : (A.n_local - 1);
    src[t] = A.codes + static_cast<uint64_t>(var) * A.code_row_bytes + G::piece_byte(col);
  }
  auto dma_stage = [&](uint32_t s, uint32_t buf) {
    const uint32_t kbyte = G::stage_byte(s);
    uint32_t* dst = lds + buf * kHhStageDwords;
#pragma unroll
    for (int t = 0; t < static_cast<int>(kHhDmaPerWave); ++t) {
      const uint32_t T = wave + kMfWaves * t;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src[t] + kbyte), (__attribute__((address_space(3))) void*)(dst + T * 256), 16, 0,
                                       0);
    }
  };

  const uint32_t sw = G::swizzle(r);
  const uint32_t oH = r * 4 + (h ^ sw);
  const uint32_t oR = r * 4 + ((2 + h) ^ sw);
  const uint32_t j_slot = q * G::kBlockSlots;
  const uint32_t v_slot = (2 + vk) * G::kBlockSlots;

  mf_v16f acc;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    acc[g] = 0.f;
  }
  uint32_t issued = 0, issue_buf = 0, read_buf = 0;
  while ((issued < n_stages) && (issued + 1 < kHhStages)) {
    dma_stage(issued, issue_buf);
    ++issued;
    issue_buf = (issue_buf + 1 == kHhStages) ? 0 : issue_buf + 1;
  }
  for (uint32_t kc = 0; kc < n_stages; ++kc) {
    // stage kc has landed in every wave's share (DMA completes in order), and every wave is done with the buffer the next issue overwrites
    wait_dma_then_barrier(kHhDmaPerWave * (issued - kc - 1));
    if (issued < n_stages) {
      dma_stage(issued, issue_buf);
      ++issued;
      issue_buf = (issue_buf + 1 == kHhStages) ? 0 : issue_buf + 1;
    }
    const mf_u4* __restrict__ st4 = reinterpret_cast<const mf_u4*>(lds + read_buf * kHhStageDwords);
    read_buf = (read_buf + 1 == kHhStages) ? 0 : read_buf + 1;
    mf_u4 jH = st4[j_slot + oH], jR = st4[j_slot + oR];
    mf_u4 vH = st4[v_slot + oH], vR = st4[v_slot + oR];
    opaque(jH, jR);
    opaque(vH, vR);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      Frag fj, fv;
      fp4_e_of_codes(jH[ks], jR[ks], fj);
      fp4_e_of_codes(vH[ks], vR[ks], fv);
      // rows of C = first variant i (A operand: the V block), columns = second variant j (B operand: the J block)
      acc = mfma_fp4g(fv, fj, acc);
    }
  }
  // ---- epilogue: straight from the registers ----
  const uint32_t j = jfirst + r;
  if ((j < A.n_local) && (j >= A.row_first) && (j < A.row_end)) {
    const uint32_t lo_j = A.lo ? A.lo[j] : 0u;
    uint32_t* out_row = A.out + static_cast<uint64_t>(j - A.row_first) * A.ld;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const uint32_t i = vfirst + (g & 3) + 8 * (g >> 2) + 4 * h;
      if ((i < j) && (i >= lo_j) && (i >= A.col_first) && (i < A.col_end)) {
        out_row[i - A.col_first] = static_cast<uint32_t>(static_cast<int32_t>(acc[g]));
      }
    }
  }
}

hipError_t launch_hethet(const HetHetArgs& a, hipStream_t stream) {
  if (!a.n_items) {
    return hipSuccess;
  }
  hipLaunchKernelGGL(pair_hethet_kernel, dim3(a.n_items), dim3(kMfWaves * 64), 0, stream, a);
  return hipGetLastError();
}

// ---- the five integers of a pair, and the bound of the hit form ---------------------------------------------------------------
// Can the pair reach min_r2?  Every root the reference accepts lies in [0, K] (it clips to that interval, plink2_ld.cc:4663-4682, and
// the degenerate branch only offers 0, K and a point between them, :4695-4706), so D = f11 + x - p q lies in [f11 - p q, f11 + K - p q]
// and r^2 = D^2 / (p q (1 - p)(1 - q)) is at most max(|lo|, |hi|)^2 over the same denominator.  |lo| and |hi| get 2^-30 of absolute
// slack: the reference's clip band is 2^-32 and the largest deviation it reports 7.9e-11 (:4664); next to it the rounding of these
// few FP64 operations (relative 1e-15 of numbers below 1) and of the caller's square root of a threshold on |r| is nothing.
// false: keep (also for pairs the host will call undefined).
__device__ __forceinline__ bool phased_hopeless(const ldp_phased_stats_t& s, double min_r2, uint32_t unsquared) {
  if (!s.valid_obs) {
    return false;
  }
  const double t = __ddiv_rn(0.5, static_cast<double>(s.valid_obs));
  const double a = static_cast<double>(s.sum0), b = static_cast<double>(s.sum1), k = static_cast<double>(s.known_dotprod), u = static_cast<double>(s.unknown_hethet);
  const double f11 = fmax(1.0 - __dmul_rn(a + b - k, t), 0.0);
  const double f12 = __dmul_rn(b - k - u, t), f21 = __dmul_rn(a - k - u, t);
  const double K = __dmul_rn(u, t);
  const double p = f11 + f12 + K, q = f11 + f21 + K;
  const double tiny = 7.105427357601002e-15;  // 2^-47 (plink2_ld.cc:4644)
  if ((p < tiny) || (1.0 - p < tiny) || (q < tiny) || (1.0 - q < tiny)) {
    return false;
  }
  const double lo = f11 - __dmul_rn(p, q), hi = lo + K;
  const double m = fmax(fabs(lo), fabs(hi)) + 9.313225746154785e-10;  // 2^-30
  const double bound = __ddiv_rn(__dmul_rn(m, m), __dmul_rn(__dmul_rn(p, q), __dmul_rn(1.0 - p, 1.0 - q)));
  const double thr = unsquared ? __dmul_rn(min_r2, min_r2) : min_r2;
  return bound < thr;  // (false for a NaN bound)
}

__global__ __launch_bounds__(256) void phased_combine_kernel(PhasedCombineArgs A) {
  const uint64_t n = static_cast<uint64_t>(A.rows) * A.cols;
  const uint64_t idx = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  uint32_t seen = 0, dropped = 0, hit_i = 0, hit_j = 0;
  ldp_phased_stats_t s = {0, 0, 0, 0, 0};
  if (idx < n) {
    const uint32_t qrow = static_cast<uint32_t>(idx / A.cols), c = static_cast<uint32_t>(idx % A.cols);
    const uint32_t j = A.row_first + qrow, i = A.col_first + c;
    const uint32_t lo_j = A.lo ? A.lo[j] : 0u;
    if ((i < j) && (i >= lo_j)) {
      const ldp_pair_stats_t T = A.tg[idx];
      const int64_t nm = T.nm;
      // non-major allele sums over the joint samples (x = 1 - g), and sum g_i g_j
      const int64_t a = nm - T.sum1, b = nm - T.sum2;
      const int64_t gg = static_cast<int64_t>(T.dot) - nm + a + b;
      const int64_t H = A.hg[idx];
      s.valid_obs = T.nm;
      if (!A.tp) {
        s.sum0 = static_cast<uint32_t>(a);
        s.sum1 = static_cast<uint32_t>(b);
        s.known_dotprod = static_cast<uint32_t>((gg - H) / 2);
        s.unknown_hethet = static_cast<uint32_t>(H);
      } else {
        // with phase rows the reference counts the MAJOR allele (g' = 2 - g: PgrGetInv1P), and its phaseinfo says "the counted allele
        // sits on the first haplotype": the file's bit where ALT is counted, its complement where REF is (pgenlib_read.cc:7023-7041)
        const ldp_pair_stats_t P = A.tp[idx];
        const int64_t gg_maj = 4 * nm - 2 * a - 2 * b + gg;
        const int64_t PP = static_cast<int64_t>(P.ssq1) + static_cast<int64_t>(P.ssq2) - static_cast<int64_t>(A.founder_ct) + static_cast<int64_t>(A.hp[idx]);
        // SS of the file's phaseinfo bits: the phase engine's tuple is in ITS records' orientation (a row with more 10 than 00 counts as ALT-major) ...
        int64_t SS = P.dot;
        if ((A.recs_p[i].flags ^ A.recs_p[j].flags) & kRecAltMajor) {
          SS = -SS;
        }
        // ... and the reference's bits differ from the file's where exactly one of the two variants counts REF
        if ((A.recs_g[i].flags ^ A.recs_g[j].flags) & kRecAltMajor) {
          SS = -SS;
        }
        const int64_t n_diff = (PP - SS) / 2;
        s.sum0 = static_cast<uint32_t>(2 * nm - a);
        s.sum1 = static_cast<uint32_t>(2 * nm - b);
        s.known_dotprod = static_cast<uint32_t>((gg_maj - H) / 2 + PP - n_diff);
        s.unknown_hethet = static_cast<uint32_t>(H - PP);
      }
      if (A.hit_count) {
        seen = 1;
        dropped = phased_hopeless(s, A.min_r2, A.unsquared) ? 1 : 0;
        hit_i = i;
        hit_j = j;
      } else if (A.out_ld) {
        A.out[static_cast<uint64_t>(qrow) * A.out_ld + c] = s;
      } else {
        A.out[A.pair_off[j] - A.band_base + (i - lo_j)] = s;
      }
    }
  }
  if (A.hit_count) {
    // survivors: ONE reservation per wave (at a low threshold every pair survives, and a 64-bit atomic per lane on one address
    // would serialise the launch), the lanes' slots by their rank among the wave's survivors
    const bool keep = seen && !dropped;
    const unsigned long long mask = __ballot(keep);
    const uint32_t lane = threadIdx.x & 63;
    if (mask) {
      const int leader = __builtin_ctzll(mask);
      unsigned long long base = 0;
      if (static_cast<int>(lane) == leader) {
        base = atomicAdd(A.hit_count, static_cast<unsigned long long>(__popcll(mask)));
      }
      const uint32_t base_lo = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(base)), leader));
      const uint32_t base_hi = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(static_cast<uint32_t>(base >> 32)), leader));
      const unsigned long long slot = ((static_cast<unsigned long long>(base_hi) << 32) | base_lo) + __popcll(mask & ((1ull << lane) - 1ull));
      if (keep && (slot < A.hit_capacity)) {
        A.hit_stats[slot] = s;
        A.hit_first[slot] = hit_i;
        A.hit_second[slot] = hit_j;
      }
    }
    seen = wave_reduce_add(seen);
    dropped = wave_reduce_add(dropped);
    if (lane == 0) {
      if (seen) {
        atomicAdd(A.hit_count + 1, static_cast<unsigned long long>(seen));
      }
      if (dropped) {
        atomicAdd(A.hit_count + 2, static_cast<unsigned long long>(dropped));
      }
    }
  }
}

hipError_t launch_phased_combine(const PhasedCombineArgs& a, hipStream_t stream) {
  const uint64_t n = static_cast<uint64_t>(a.rows) * a.cols;
  if (!n) {
    return hipSuccess;
  }
  const uint64_t blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffull) {
    return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL(phased_combine_kernel, dim3(static_cast<uint32_t>(blocks)), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace ldp
