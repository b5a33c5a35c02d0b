// ldp_engine_king.cpp -- ldp_king_counts_block() / ldp_king_block_hits(): the KING-robust counts of the sample pairs of a block, from the
// resident 2-bit image (ldp_king.hip).  Contract, states and refusals are those of resident_runs() (ldp_engine.cpp),
// with the image, behind the call's own argument checks (the debug form answers under the public call's name).  Each run of owned rows is
// cut into slabs; per slab the row samples' and the column samples' strips are written (one set when both ranges start in the same group of
// samples and the rows reach at least as far) and one pair launch adds the slab's counts to the block's.
// (host runtime behind include/ldprune_hip.h; ldp_engine.cpp has the overview)
#include "ldp_engine_internal.h"
#include "ldp_king_device.h"

namespace {

static_assert(sizeof(ldp_king_counts_t) == 20 && sizeof(ldp_king_hit) == 28, "the kernels write these layouts");

struct KingRequest {
  uint32_t first_variant, n;
  const uint8_t* include;
  uint32_t row_first, row_ct, col_first, col_ct;
};

// dense != NULL: the dense form; otherwise the hit form.  slab_variants: 0 = chosen from the sample counts
int king_impl(ldp_engine* e, const char* who, const KingRequest& q, ldp_king_counts_t* dense, uint64_t ld_elems, bool hit_form, double min_kinship, ldp_king_hit* hits,
              uint64_t capacity, uint64_t* count, uint32_t slab_variants, double* ms_kernel, uint64_t* pair_variants) {
  if (!e) {
    return LDP_ERR_INVALID;
  }
  if (ms_kernel) {
    *ms_kernel = 0.0;
  }
  if (pair_variants) {
    *pair_variants = 0;
  }
  if (count) {
    *count = 0;
  }
  if (!e->planned) {
    return fail(e, LDP_ERR_STATE, "ldp_set_variants*() and the loads first");
  }
  if (hit_form) {
    if (!count || (capacity && !hits)) {
      return fail(e, LDP_ERR_INVALID, "count is NULL, or capacity without out");
    }
  } else if (!dense && q.row_ct && q.col_ct) {
    return fail(e, LDP_ERR_INVALID, "out is NULL");
  } else if (ld_elems < q.col_ct) {
    return fail(e, LDP_ERR_INVALID, "ld_elems is smaller than col_ct");
  }
  const uint32_t founder_ct = e->P.founder_ct;
  if ((static_cast<uint64_t>(q.row_first) + q.row_ct > founder_ct) || (static_cast<uint64_t>(q.col_first) + q.col_ct > founder_ct)) {
    return fail(e, LDP_ERR_INVALID, "sample range beyond founder_ct");
  }
  if (slab_variants && ((slab_variants % ldp::kKingSlabMin) || (slab_variants > ldp::kKingSlabMax))) {
    return fail(e, LDP_ERR_INVALID, "slab_variants: a multiple of 256, at most 65536");
  }
  std::vector<ResidentRun> runs;
  int rc = resident_runs(e, who, q.first_variant, q.n, true, &runs);
  if (rc) {
    return rc;
  }
  if (dense) {
    for (uint32_t r = 0; r < q.row_ct; ++r) {
      memset(dense + static_cast<uint64_t>(r) * ld_elems, 0, static_cast<size_t>(q.col_ct) * sizeof(ldp_king_counts_t));
    }
  }
  // pairs col < row of the block
  uint64_t pairs = 0;
  for (uint32_t r = 0; r < q.row_ct; ++r) {
    const uint64_t row = static_cast<uint64_t>(q.row_first) + r;
    if (row > q.col_first) {
      pairs += std::min<uint64_t>(row - q.col_first, q.col_ct);
    }
  }
  const bool work = q.n && pairs;
  if (!work && !hit_form) {
    return LDP_OK;
  }
  if (!pairs) {
    return LDP_OK;  // (the hit form without a pair: no hit)
  }
  rc = begin_resident_read(e);
  if (rc) {
    return rc;
  }
  const uint32_t G = ldp::kKingStripSamples;
  const uint32_t row_end = q.row_first + q.row_ct, col_end = q.col_first + q.col_ct;
  const uint32_t a_base = q.row_first / G * G, b_base = q.col_first / G * G;
  const uint32_t a_blocks = (row_end - a_base + G - 1) / G;
  // columns at or beyond the last row are in no pair
  const uint32_t col_end_used = std::min(col_end, row_end);
  const uint32_t b_blocks = (col_end_used - b_base + G - 1) / G;
  const bool shared = (a_base == b_base) && (a_blocks >= b_blocks);
  const uint32_t K = slab_variants ? slab_variants : ldp::king_slab_variants(q.row_ct, q.col_ct);
  const size_t strip_bytes = K / 4;
  const size_t a_bytes = static_cast<size_t>(a_blocks) * G * strip_bytes, b_bytes = shared ? 0 : static_cast<size_t>(b_blocks) * G * strip_bytes;
  const size_t counts_bytes = static_cast<size_t>(q.row_ct) * q.col_ct * sizeof(ldp_king_counts_t);
  DevBuf d_strips, d_counts, d_inc, d_hits;
  EventSet<2> ev;
  HIP_TRY(e, ev.create());
  HIP_TRY(e, hipMalloc(&d_counts.p, counts_bytes));
  HIP_TRY(e, hipMemsetAsync(d_counts.p, 0, counts_bytes, e->stream));
  uint64_t included = q.n;
  if (work) {
    HIP_TRY(e, hipMalloc(&d_strips.p, a_bytes + b_bytes));
    if (q.include) {
      HIP_TRY(e, hipMalloc(&d_inc.p, q.n));
      HIP_TRY(e, hipMemcpyAsync(d_inc.p, q.include, q.n, hipMemcpyHostToDevice, e->stream));
      included = 0;
      for (uint32_t k = 0; k < q.n; ++k) {
        included += q.include[k] != 0;
      }
    }
  }
  uint8_t* strips_a = d_strips.as<uint8_t>();
  uint8_t* strips_b = shared ? strips_a : strips_a + a_bytes;
  HIP_TRY(e, hipEventRecord(ev.ev[0], e->stream));
  if (work) {
    for (const ResidentRun& r : runs) {
      for (uint32_t s = 0; s < r.ct; s += K) {
        const uint32_t rows = std::min(K, r.ct - s);
        // (a short last slab runs its whole length only up to the next 256 variants: the rest would be code 11 against code 11)
        const uint32_t k_len = (rows + ldp::kKingSlabMin - 1) / ldp::kKingSlabMin * ldp::kKingSlabMin;
        const uint8_t* inc = d_inc.p ? d_inc.as<uint8_t>() + r.off + s : nullptr;
        hipError_t krc = ldp::launch_king_transpose(e->d_codes, e->code_row_bytes, static_cast<uint64_t>(r.l_first) + s, rows, inc, founder_ct, a_base, a_blocks, strips_a, k_len,
                                                    e->stream);
        if ((krc == hipSuccess) && !shared) {
          krc = ldp::launch_king_transpose(e->d_codes, e->code_row_bytes, static_cast<uint64_t>(r.l_first) + s, rows, inc, founder_ct, b_base, b_blocks, strips_b, k_len, e->stream);
        }
        if (krc != hipSuccess) {
          return hipfail(e, krc, "king_transpose_kernel launch");
        }
        krc = ldp::launch_king_pairs(strips_a, strips_b, k_len, a_base, b_base, q.row_first, q.row_ct, q.col_first, col_end_used - q.col_first, d_counts.p, q.col_ct, e->stream);
        if (krc != hipSuccess) {
          return hipfail(e, krc, "king_pair_kernel launch");
        }
      }
    }
  }
  if (hit_form) {
    const size_t hit_bytes = static_cast<size_t>(capacity) * sizeof(ldp_king_hit) + 8;
    HIP_TRY(e, hipMalloc(&d_hits.p, hit_bytes));
    uint64_t* d_count = d_hits.as<uint64_t>();  // the counter first, the list behind it (8-byte aligned, the hits need 4)
    ldp_king_hit* d_list = reinterpret_cast<ldp_king_hit*>(d_hits.as<uint8_t>() + 8);
    HIP_TRY(e, hipMemsetAsync(d_count, 0, 8, e->stream));
    const hipError_t krc = ldp::launch_king_hits(d_counts.p, q.col_ct, q.row_first, q.row_ct, q.col_first, q.col_ct, min_kinship, d_list, capacity, d_count, e->stream);
    if (krc != hipSuccess) {
      return hipfail(e, krc, "king_hits_kernel launch");
    }
    HIP_TRY(e, hipEventRecord(ev.ev[1], e->stream));
    HIP_TRY(e, hipMemcpyAsync(count, d_count, 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
    const uint64_t got = std::min<uint64_t>(*count, capacity);
    if (got) {
      HIP_TRY(e, hipMemcpyAsync(hits, d_list, static_cast<size_t>(got) * sizeof(ldp_king_hit), hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(e, hipStreamSynchronize(e->stream));
    }
  } else {
    HIP_TRY(e, hipEventRecord(ev.ev[1], e->stream));
    HIP_TRY(e, hipMemcpy2DAsync(dense, static_cast<size_t>(ld_elems) * sizeof(ldp_king_counts_t), d_counts.p, static_cast<size_t>(q.col_ct) * sizeof(ldp_king_counts_t),
                                static_cast<size_t>(q.col_ct) * sizeof(ldp_king_counts_t), q.row_ct, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(e, hipStreamSynchronize(e->stream));
  }
  if (ms_kernel) {
    *ms_kernel = ev.elapsed_ms(0, 1);
  }
  if (pair_variants) {
    *pair_variants = pairs * included;
  }
  return LDP_OK;
}

}  // namespace

extern "C" {

int ldp_king_counts_block(ldp_engine* e, uint32_t first_variant, uint32_t n, const uint8_t* include, uint32_t row_first, uint32_t row_ct, uint32_t col_first, uint32_t col_ct,
                          ldp_king_counts_t* out, uint64_t ld_elems) {
  const KingRequest q = {first_variant, n, include, row_first, row_ct, col_first, col_ct};
  return king_impl(e, "ldp_king_counts_block()", q, out, ld_elems, false, 0.0, nullptr, 0, nullptr, 0, nullptr, nullptr);
}

int ldp_king_block_hits(ldp_engine* e, uint32_t first_variant, uint32_t n, const uint8_t* include, uint32_t row_first, uint32_t row_ct, uint32_t col_first, uint32_t col_ct,
                        double min_kinship, ldp_king_hit* out, uint64_t capacity, uint64_t* count) {
  const KingRequest q = {first_variant, n, include, row_first, row_ct, col_first, col_ct};
  return king_impl(e, "ldp_king_block_hits()", q, nullptr, 0, true, min_kinship, out, capacity, count, 0, nullptr, nullptr);
}

int ldp_debug_king_counts_block(ldp_engine* e, uint32_t first_variant, uint32_t n, const uint8_t* include, uint32_t row_first, uint32_t row_ct, uint32_t col_first,
                                uint32_t col_ct, ldp_king_counts_t* out, uint64_t ld_elems, uint32_t slab_variants, double* ms_kernel, uint64_t* pair_variants) {
  const KingRequest q = {first_variant, n, include, row_first, row_ct, col_first, col_ct};
  return king_impl(e, "ldp_king_counts_block()", q, out, ld_elems, false, 0.0, nullptr, 0, nullptr, slab_variants, ms_kernel, pair_variants);
}

}  // extern "C"
