// ldp_engine_phased.cpp -- --r2-phased / --r-phased: the five integers of every pair of a block or a band (ldp_phased_stats_t), dense
// or filtered on the device by the bound of ldp_r2_phased_band_hits() (host runtime behind include/ldprune_hip.h; the kernels and the
// identities are in ldp_pair_phased.hip, the floating-point tail in ldp_phased_ld.cpp)
#include "ldp_engine_internal.h"

namespace ldph LDP_HIDDEN {

// what the last ldp_r2_phased_* call did (ldp_debug_get_phased_filter)
void remember_phased(ldp_engine* e, const PhasedFilterStats& st) { e->phased_last = st; }

struct PhasedHits {
  double min_r2;
  int unsquared;
  ldp_phased_stats_t* stats;
  uint32_t* first;
  uint32_t* second;
  uint64_t capacity;
  uint64_t* count;
};

// the 64 x 64 workgroups of pair_hethet_kernel that hold a pair (i, j) with j in [r0, r0 + rows), i in [c0, c1), lo[j] <= i < j
void plan_hethet(const uint32_t* lo, uint32_t r0, uint32_t rows, uint32_t c0, uint32_t c1, std::vector<HetHetItem>* items) {
  items->clear();
  const uint32_t r_end = r0 + rows;
  for (uint32_t jv = r0; jv < r_end; jv += 64) {
    const uint32_t j_last = std::min(jv + 64, r_end) - 1;
    uint32_t i_first = c0;
    if (lo) {
      uint32_t m = 0xffffffffu;
      for (uint32_t j = jv; j <= j_last; ++j) {
        m = std::min(m, lo[j]);
      }
      i_first = std::max(c0, m);
    }
    const uint32_t i_end = std::min(c1, j_last);  // i < j <= j_last
    for (uint32_t vv = i_first; vv < i_end; vv += 64) {
      items->push_back({jv, vv});
    }
  }
}

// what the double-heterozygote launches of ONE call on one engine reuse from chunk to chunk: the item list's device buffer (grown
// when a chunk needs more) and the pair of timing events
struct HetHetScratch {
  DevBuf items;
  size_t capacity = 0;
  EventSet<2> ev;
  bool ready = false;
  bool timed = false;  // the events bracket a launch whose time has not been read yet
  bool marked = false; // ev[1] has been recorded behind this chunk's work on the engine's stream (the launch, or the memset alone)
};

// H of one engine for a dense chunk, into d_h ([rows][cols], zeroed here), queued on the engine's stream: no synchronisation here.
// The caller reads the launch's time with hethet_time() once the stream has been synchronised.
int hethet_chunk(ldp_engine* e, HetHetScratch* sc, uint32_t r0, uint32_t rows, uint32_t c0, uint32_t c1, bool band, uint32_t* d_h) {
  const uint32_t cols = c1 - c0;
  HIP_TRY(e, hipSetDevice(e->device));
  if (!sc->ready) {
    HIP_TRY(e, sc->ev.create());
    sc->ready = true;
  }
  HIP_TRY(e, hipMemsetAsync(d_h, 0, static_cast<uint64_t>(rows) * cols * sizeof(uint32_t), e->stream));
  std::vector<HetHetItem> items;
  plan_hethet(band ? e->lo_local.data() : nullptr, r0, rows, c0, c1, &items);
  sc->marked = false;
  if (items.empty()) {
    // no pair in this chunk: d_h stays zero and nobody reads it, but whoever waits for this engine's chunk still gets an event to wait for
    HIP_TRY(e, hipEventRecord(sc->ev.ev[1], e->stream));
    sc->marked = true;
    return LDP_OK;
  }
  if (items.size() > sc->capacity) {
    if (sc->items.p) {
      HIP_TRY(e, hipFree(sc->items.p));
      sc->items.p = nullptr;
    }
    sc->capacity = items.size() + items.size() / 2;
    HIP_TRY(e, hipMalloc(&sc->items.p, sc->capacity * sizeof(HetHetItem)));
  }
  // (a blocking copy: the list is a host vector of this scope, and the stream is idle here -- the six-integer call before this one ended
  // with its synchronisation -- so the previous chunk's launch is done with the buffer)
  HIP_TRY(e, hipMemcpy(sc->items.p, items.data(), items.size() * sizeof(HetHetItem), hipMemcpyHostToDevice));
  HetHetArgs A;
  A.codes = e->d_codes;
  A.code_row_bytes = e->code_row_bytes;
  A.founder_ct = e->P.founder_ct;
  A.n_local = e->local_ct;
  A.lo = band ? e->d_lo : nullptr;
  A.items = sc->items.as<HetHetItem>();
  A.n_items = static_cast<uint32_t>(items.size());
  A.row_first = r0;
  A.row_end = r0 + rows;
  A.col_first = c0;
  A.col_end = c1;
  A.out = d_h;
  A.ld = cols;
  HIP_TRY(e, hipEventRecord(sc->ev.ev[0], e->stream));
  const hipError_t krc = launch_hethet(A, e->stream);
  if (krc != hipSuccess) {
    return hipfail(e, krc, "pair_hethet_kernel launch");
  }
  HIP_TRY(e, hipEventRecord(sc->ev.ev[1], e->stream));
  sc->timed = true;
  sc->marked = true;
  return LDP_OK;
}

int hethet_time(ldp_engine* e, HetHetScratch* sc, double* ms) {
  if (sc->timed) {
    float t = 0.f;
    HIP_TRY(e, hipEventElapsedTime(&t, sc->ev.ev[0], sc->ev.ev[1]));
    *ms += t;
    sc->timed = false;
  }
  return LDP_OK;
}

int phased_ready(ldp_engine* e, ldp_engine* x, bool band, const char* who) {
  if (!x->planned || !(band ? x->band_r2_mode : x->matrix_mode)) {
    return fail(e, LDP_ERR_STATE, std::string(who) + (band ? "ldp_set_variants_vcor() first" : "ldp_set_variants_matrix() first"));
  }
  if ((x->world > 1) || (x->local_ct != x->variant_ct)) {
    return fail(e, LDP_ERR_UNSUPPORTED, std::string(who) + "the phased statistics do not run on a sharded engine");
  }
  const int rc = ensure_device_plan(x);
  if (rc) {
    return (x == e) ? rc : fail(e, rc, std::string(who) + ldp_last_error(x));
  }
  if (!x->codes_format) {
    return fail(e, LDP_ERR_UNSUPPORTED, std::string(who) + "the phased statistics need the matrix-pipe kernels (option pair_mfma)");
  }
  for (uint32_t l = 0; l < x->local_ct; ++l) {
    if (!x->loaded[l]) {
      return fail(e, LDP_ERR_STATE, std::string(who) + "genotypes missing for a variant (ldp_load_genotypes)");
    }
  }
  return LDP_OK;
}

// band == false: the dense block [row_first, +row_ct) x [col_first, +col_ct) into out (leading dimension ld_or_cap);
// band == true: the band's pairs of second variants [row_first, +row_ct), into out (capacity ld_or_cap) or filtered into *hits
int phased_impl(ldp_engine* e, ldp_engine* ph, bool band, uint32_t row_first, uint32_t row_ct, uint32_t col_first, uint32_t col_ct, ldp_phased_stats_t* out,
                uint64_t ld_or_cap, const PhasedHits* hits) {
  if (!e) {
    return LDP_ERR_INVALID;
  }
  if (hits) {
    if (!hits->count || (hits->capacity && (!hits->stats || !hits->first || !hits->second))) {
      return fail(e, LDP_ERR_INVALID, "hit buffers missing");
    }
    *hits->count = 0;
  }
  // the counts are f32 accumulators: exact below 2^24 (no popcount form of the double-heterozygote product exists)
  if ((e->P.founder_ct > ldp_matrix_pipe_max_founders()) || (ph && (ph->P.founder_ct > ldp_matrix_pipe_max_founders()))) {
    return fail(e, LDP_ERR_UNSUPPORTED, "the phased statistics run on the matrix pipe only: more founders than ldp_matrix_pipe_max_founders()");
  }
  if (ph && ((ph == e) || (ph->P.founder_ct != e->P.founder_ct))) {
    return fail(e, LDP_ERR_INVALID, "the phase engine must be a second engine over the same founders");
  }
  int rc = phased_ready(e, e, band, "");
  if (rc) {
    return rc;
  }
  if (ph) {
    if ((rc = phased_ready(e, ph, band, "phase engine: "))) {
      return rc;
    }
    if ((ph->variant_ct != e->variant_ct) || (ph->device != e->device) || (band && (ph->lo_local != e->lo_local))) {
      return fail(e, LDP_ERR_INVALID, "the phase engine must hold the same variants under the same plan on the same device");
    }
  }
  const uint32_t m = e->variant_ct;
  if ((static_cast<uint64_t>(row_first) + row_ct > m) || (!band && (static_cast<uint64_t>(col_first) + col_ct > m))) {
    return fail(e, LDP_ERR_INVALID, "row / column range out of bounds");
  }
  const uint32_t row_end = row_first + row_ct;
  uint64_t band_elems = 0;
  if (band) {
    band_elems = e->pair_off[row_end] - e->pair_off[row_first];
    if (!hits && (band_elems > ld_or_cap)) {
      return fail(e, LDP_ERR_INVALID, "output buffer smaller than the rows' candidate pair count");
    }
    if (!hits && band_elems && !out) {
      return fail(e, LDP_ERR_INVALID, "output buffer is NULL");
    }
  } else {
    if (row_ct && col_ct && (!out || (ld_or_cap < col_ct))) {
      return fail(e, LDP_ERR_INVALID, "output buffer / leading dimension out of bounds");
    }
    for (uint32_t q = 0; col_ct && (q < row_ct); ++q) {  // (zero where there is no pair)
      memset(out + static_cast<uint64_t>(q) * ld_or_cap, 0, static_cast<size_t>(col_ct) * sizeof(ldp_phased_stats_t));
    }
  }
  PhasedFilterStats fst;
  if (!row_ct || (band ? !band_elems : !col_ct)) {
    remember_phased(e, fst);
    return LDP_OK;
  }
  HIP_TRY(e, hipSetDevice(e->device));
  const uint32_t* lo = band ? e->lo_local.data() : nullptr;
  const uint32_t col_end = band ? row_end : (col_first + col_ct);
  // row chunks: rows are cut so that a chunk's dense scratch -- six integers and H per engine, the five integers going out -- is about
  // 512 MiB at the chunk's column count.  Columns are NOT cut: a chunk is never shorter than 64 rows, so a block wider than ~100,000
  // columns takes more (64 x col_ct x 48-76 bytes); the caller of the block form bounds that with col_ct.
  // The band form pays for this layout: a chunk of R rows is R x (R + window) dense entries for R x window wanted, in the six-integer
  // launches and in the combine kernel (only pair_hethet_kernel's plan skips what lies in front of the window starts).
  const uint64_t per_elem = (ph ? 2 : 1) * (sizeof(ldp_pair_stats_t) + sizeof(uint32_t)) + sizeof(ldp_phased_stats_t);
  const uint64_t budget = (512ull << 20) / per_elem;
  auto chunk_cols = [&](uint32_t r0, uint32_t rows, uint32_t* c0, uint32_t* c1) {
    uint32_t first = band ? 0xffffffffu : col_first;
    for (uint32_t j = r0; band && (j < r0 + rows); ++j) {
      first = std::min(first, lo[j]);
    }
    *c0 = first;
    *c1 = std::min(col_end, r0 + rows - 1);  // i < j <= r0 + rows - 1
  };
  struct Chunk {
    uint32_t r0, rows, c0, c1;
  };
  std::vector<Chunk> chunks;
  uint64_t max_elems = 0, max_band = 0;
  for (uint32_t r0 = row_first; r0 < row_end;) {
    uint32_t rows = std::min<uint32_t>(row_end - r0, 8192), c0, c1;
    for (;;) {
      chunk_cols(r0, rows, &c0, &c1);
      if ((rows <= 64) || (c0 >= c1) || (static_cast<uint64_t>(rows) * (c1 - c0) <= budget)) {
        break;
      }
      rows = std::max<uint32_t>(64, (rows / 2) & ~63u);
    }
    if (c0 < c1) {
      chunks.push_back({r0, rows, c0, c1});
      max_elems = std::max(max_elems, static_cast<uint64_t>(rows) * (c1 - c0));
      if (band) {
        max_band = std::max(max_band, e->pair_off[r0 + rows] - e->pair_off[r0]);
      }
    }
    r0 += rows;
  }
  if (chunks.empty()) {
    remember_phased(e, fst);
    return LDP_OK;
  }
  DevBuf tg, hg, tp, hp, d_out, d_hs, d_hf, d_h2, d_ctr;
  HIP_TRY(e, hipMalloc(&tg.p, max_elems * sizeof(ldp_pair_stats_t)));
  HIP_TRY(e, hipMalloc(&hg.p, max_elems * sizeof(uint32_t)));
  if (ph) {
    HIP_TRY(e, hipMalloc(&tp.p, max_elems * sizeof(ldp_pair_stats_t)));
    HIP_TRY(e, hipMalloc(&hp.p, max_elems * sizeof(uint32_t)));
  }
  if (hits) {
    const uint64_t cap = std::max<uint64_t>(hits->capacity, 1);
    HIP_TRY(e, hipMalloc(&d_hs.p, cap * sizeof(ldp_phased_stats_t)));
    HIP_TRY(e, hipMalloc(&d_hf.p, cap * sizeof(uint32_t)));
    HIP_TRY(e, hipMalloc(&d_h2.p, cap * sizeof(uint32_t)));
    HIP_TRY(e, hipMalloc(&d_ctr.p, 3 * sizeof(unsigned long long)));
    HIP_TRY(e, hipMemsetAsync(d_ctr.p, 0, 3 * sizeof(unsigned long long), e->stream));
  } else {
    HIP_TRY(e, hipMalloc(&d_out.p, (band ? max_band : max_elems) * sizeof(ldp_phased_stats_t)));
  }
  HetHetScratch sc_g, sc_p;
  for (const Chunk& ch : chunks) {
    const uint32_t cols = ch.c1 - ch.c0;
    // the six integers of both engines (left on the device; each call synchronises its engine's stream), then H
    if ((rc = r2_rows_impl(e, ch.r0, ch.rows, 2, tg.p, cols, nullptr, ch.c0, ch.c1, true, true))) {
      return rc;
    }
    fst.ms_tuples += e->ctr.ms_pair_kernel;
    if ((rc = hethet_chunk(e, &sc_g, ch.r0, ch.rows, ch.c0, ch.c1, band, hg.as<uint32_t>()))) {
      return rc;
    }
    if (ph) {
      if ((rc = r2_rows_impl(ph, ch.r0, ch.rows, 2, tp.p, cols, nullptr, ch.c0, ch.c1, true, true))) {
        return fail(e, rc, std::string("phase engine: ") + ldp_last_error(ph));
      }
      fst.ms_tuples += ph->ctr.ms_pair_kernel;
      if ((rc = hethet_chunk(ph, &sc_p, ch.r0, ch.rows, ch.c0, ch.c1, band, hp.as<uint32_t>()))) {
        return fail(e, rc, std::string("phase engine: ") + ldp_last_error(ph));
      }
      // the combine kernel on e's stream reads what ph's stream is still writing
      if (sc_p.marked && (ph->stream != e->stream)) {
        HIP_TRY(e, hipStreamWaitEvent(e->stream, sc_p.ev.ev[1], 0));
      }
    }
    PhasedCombineArgs C;
    C.tg = tg.as<ldp_pair_stats_t>();
    C.hg = hg.as<uint32_t>();
    C.tp = ph ? tp.as<ldp_pair_stats_t>() : nullptr;
    C.hp = ph ? hp.as<uint32_t>() : nullptr;
    C.recs_g = e->d_recs;
    C.recs_p = ph ? ph->d_recs : nullptr;
    C.lo = band ? e->d_lo : nullptr;
    C.rows = ch.rows;
    C.cols = cols;
    C.row_first = ch.r0;
    C.col_first = ch.c0;
    C.founder_ct = e->P.founder_ct;
    C.out = d_out.as<ldp_phased_stats_t>();
    C.out_ld = band ? 0 : cols;
    C.pair_off = band ? e->d_pair_off : nullptr;
    C.band_base = band ? e->pair_off[ch.r0] : 0;
    C.hit_stats = d_hs.as<ldp_phased_stats_t>();
    C.hit_first = d_hf.as<uint32_t>();
    C.hit_second = d_h2.as<uint32_t>();
    C.hit_capacity = hits ? hits->capacity : 0;
    C.hit_count = hits ? d_ctr.as<unsigned long long>() : nullptr;
    C.min_r2 = hits ? hits->min_r2 : 0.0;
    C.unsquared = (hits && hits->unsquared) ? 1u : 0u;
    const uint64_t chunk_band = band ? (e->pair_off[ch.r0 + ch.rows] - e->pair_off[ch.r0]) : 0;
    if (!hits) {
      HIP_TRY(e, hipMemsetAsync(d_out.p, 0, (band ? chunk_band : static_cast<uint64_t>(ch.rows) * cols) * sizeof(ldp_phased_stats_t), e->stream));
    }
    const hipError_t krc = launch_phased_combine(C, e->stream);
    if (krc != hipSuccess) {
      return hipfail(e, krc, "phased_combine_kernel launch");
    }
    if (hits) {
      HIP_TRY(e, hipStreamSynchronize(e->stream));  // (the next chunk overwrites the scratch from both engines' streams)
    } else if (band) {
      HIP_TRY(e, hipMemcpyAsync(out + (e->pair_off[ch.r0] - e->pair_off[row_first]), d_out.p, chunk_band * sizeof(ldp_phased_stats_t), hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(e, hipStreamSynchronize(e->stream));
    } else {
      HIP_TRY(e, hipMemcpy2DAsync(out + static_cast<uint64_t>(ch.r0 - row_first) * ld_or_cap + (ch.c0 - col_first), ld_or_cap * sizeof(ldp_phased_stats_t), d_out.p,
                                  static_cast<size_t>(cols) * sizeof(ldp_phased_stats_t), static_cast<size_t>(cols) * sizeof(ldp_phased_stats_t), ch.rows,
                                  hipMemcpyDeviceToHost, e->stream));
      HIP_TRY(e, hipStreamSynchronize(e->stream));
    }
    // (e's stream waited for the phase engine's launch: both pairs of events have completed)
    if ((rc = hethet_time(e, &sc_g, &fst.ms_hethet)) || (ph && (rc = hethet_time(ph, &sc_p, &fst.ms_hethet)))) {
      return rc;
    }
  }
  if (hits) {
    unsigned long long c3[3] = {0, 0, 0};
    HIP_TRY(e, hipMemcpy(c3, d_ctr.p, sizeof(c3), hipMemcpyDeviceToHost));
    *hits->count = c3[0];
    fst.seen = c3[1];
    fst.dropped = c3[2];
    const uint64_t stored = std::min<uint64_t>(c3[0], hits->capacity);
    if (stored) {
      HIP_TRY(e, hipMemcpy(hits->stats, d_hs.p, stored * sizeof(ldp_phased_stats_t), hipMemcpyDeviceToHost));
      HIP_TRY(e, hipMemcpy(hits->first, d_hf.p, stored * sizeof(uint32_t), hipMemcpyDeviceToHost));
      HIP_TRY(e, hipMemcpy(hits->second, d_h2.p, stored * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
  }
  remember_phased(e, fst);
  return LDP_OK;
}
}  // namespace ldph

extern "C" {

int ldp_r2_phased_stats_block(ldp_engine* e, ldp_engine* phase, uint32_t row_first, uint32_t row_ct, uint32_t col_first, uint32_t col_ct, ldp_phased_stats_t* out,
                              uint64_t ld_elems) {
  return phased_impl(e, phase, false, row_first, row_ct, col_first, col_ct, out, ld_elems, nullptr);
}

int ldp_r2_phased_band_stats(ldp_engine* e, ldp_engine* phase, uint32_t row_first, uint32_t row_ct, ldp_phased_stats_t* out, uint64_t capacity) {
  return phased_impl(e, phase, true, row_first, row_ct, 0, 0, out, capacity, nullptr);
}

int ldp_r2_phased_band_hits(ldp_engine* e, ldp_engine* phase, uint32_t row_first, uint32_t row_ct, double min_r2, int unsquared, ldp_phased_stats_t* out_stats,
                            uint32_t* out_first, uint32_t* out_second, uint64_t capacity, uint64_t* count) {
  const PhasedHits h{min_r2, unsquared, out_stats, out_first, out_second, capacity, count};
  return phased_impl(e, phase, true, row_first, row_ct, 0, 0, nullptr, 0, &h);
}

int ldp_debug_get_phased_filter(const ldp_engine* e, uint64_t* pairs_seen, uint64_t* pairs_dropped, double* ms_hethet, double* ms_tuples) {
  if (!e) {
    return LDP_ERR_INVALID;
  }
  const PhasedFilterStats& st = e->phased_last;
  if (pairs_seen) {
    *pairs_seen = st.seen;
  }
  if (pairs_dropped) {
    *pairs_dropped = st.dropped;
  }
  if (ms_hethet) {
    *ms_hethet = st.ms_hethet;
  }
  if (ms_tuples) {
    *ms_tuples = st.ms_tuples;
  }
  return LDP_OK;
}

}  // extern "C"
