/* ldprune_hip_debug.h -- test hooks, kernel-selection switches and the benchmark generator of libldprune_hip.so.
 *
 * Nothing here belongs to the drop-in boundary (include/ldprune_hip.h): a host that prunes never calls any of it.  The entry points
 * exist for the parity tests (host-only replay and plan views that run without a GPU), for measurements (switching kernels on one
 * engine) and for bench.py (a deterministic genotype generator, so that the 1.25 TB matrix of the metric never has to exist on disk).
 */
#ifndef LDPRUNE_HIP_DEBUG_H
#define LDPRUNE_HIP_DEBUG_H

#include "ldprune_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only replay of the greedy scan (plink2_ld.cc:931-1100) from a caller-supplied list of the candidate
 * pairs whose predicate is TRUE (global variant indices, first < second, each inside the band).  Needs
 * variant records (ldp_debug_set_variant_recs, for the monomorphic flags) and maj_freqs.  No GPU is
 * touched: this is how the host logic is tested on a CPU-only machine. */
int ldp_debug_set_variant_recs(ldp_engine* e, const ldp_variant_rec* recs);
int ldp_debug_replay_pairs(ldp_engine* e, uint64_t n_true, const uint32_t* first, const uint32_t* second, uint64_t* removed);
/* The decisions of the last run, one byte (0 / 1) per candidate pair in the order of ldp_run_with_stats()'s `stats` array (ldp_get_band()):
 * the dense predicate rows every pair kernel sets its bits in, copied back from the device as they stand after ldp_run() or
 * ldp_run_with_stats() -- the production run's, with early termination, routes and launch groups as they were.  *outside_band (optional)
 * receives the number of bits set in the rows' first / last words OUTSIDE the band (a kernel that writes there is wrong; they are not
 * part of `out`).  LDP_ERR_STATE when no run has completed since the last load (the rows are cleared group by group as launches are
 * queued), LDP_ERR_INVALID when capacity < candidate pairs, LDP_ERR_UNSUPPORTED on a sharded engine.  Reads finished results only. */
int ldp_debug_get_pred(ldp_engine* e, uint8_t* out, uint64_t capacity, uint64_t* outside_band);
/* What the host replay of the last ldp_run() READ: the predicate rows as the device compacted them (csrc/ldp_pred_csr.hip) into pinned host
 * memory.  meta receives two words per local row j -- (first entry, entries) --, ent two words per entry in use -- (word index inside the
 * row, bits; bit b of word w of row j: the pair (32 ((lo[j] >> 5) + w) + b, j)) --; a row's entries ascend by word index, the rows' runs
 * lie in no particular order.  *n_rows: the rows (shard-local variants), *used: the entries in use (the device's count, capped by the
 * capacity), *device_count: the non-zero words the device counted (one copy of the counter, after waiting for the engine's stream),
 * *overflow: 1 when that exceeded *capacity (the entries in force, option "csr_capacity") -- the run then replayed the dense rows instead,
 * and meta / ent are incomplete --, *overflow_runs: the runs of this engine that fell back so.  Any output pointer may be NULL; meta and
 * ent both NULL only reports the counts.  Reads finished results only: no kernel is launched, nothing a run does changes.
 * LDP_ERR_STATE when the last completed run returned no compacted rows -- no run since the last load, an inspection run
 * (ldp_run_with_stats), an engine with "pred_csr" 0 --, LDP_ERR_INVALID when meta_capacity < rows or ent_capacity < entries in use (both in
 * pairs of words), LDP_ERR_UNSUPPORTED on a sharded engine. */
int ldp_debug_get_pred_csr(ldp_engine* e, uint32_t* meta, uint64_t meta_capacity, uint32_t* ent, uint64_t ent_capacity, uint32_t* n_rows, uint64_t* used,
                           uint64_t* device_count, uint32_t* overflow, uint64_t* capacity, uint32_t* overflow_runs);
/* Kernel-selection switches of ONE engine, for tests and measurements (the defaults are what production runs use).  The shipped
 * library reads NO environment variable (csrc/ldp_env.h): this call is the only way to switch anything, engine by engine; only the
 * measurement build (-DLDP_MEASURE, lib/libldprune_hip_measure.so, tools/) presets them from LDP_* variables.  name:
 *   "early_exit"      0/1: checkpoints that drop provably sub-threshold products
 *   "pair_mfma"       0/1: matrix-pipe kernels on the 2-bit code image; 0 = the popcount kernels on bit-planes (before ldp_set_variants*())
 *   "pair_sparse"     0/1: the interval epilogue for rows with a few missing calls
 *   "sparse_frac"     mean missing fraction up to which a launch takes it
 *   "pair_four"       0/1: prune launches over rows with more missing calls than that multiply four products per pair and take the
 *                     two sums of squares from per-variant intervals (exact count for the few pairs they leave open); 0 = all six
 *   "pair_gu"         0/1: the four-product form's operands are allele counts and missing flags (default 1; exact up to 1,800,000
 *                     founders, engines with more use 0 by themselves); 0 = the +-2 coded x and the call flags n of rounds 2-3
 *   "pair_four_tiles" 0/1: ... and in wide bands (subcontigs with the tile plan) that form runs over quarter tiles instead of the
 *                     parallelogram plan (default 1)
 *   "orient_rows"     0/1: the count pass stores a row whose ALT allele is the major one with codes 00 <-> 10 swapped, so that every row of the image is
 *                     major-allele-oriented (default 1: hom-major = operand 0 is the cheapest genotype for the power-capped pair kernels; the record
 *                     says so in flags bit 3); 0 = rows stay as the input had them (rounds 2-5)
 *   "pred_csr"        0/1: prune runs return the predicate rows as their non-zero words, compacted on the device and written straight into pinned host
 *                     memory (default 1); 0 = the dense rows are copied back whole, as in rounds 1-5
 *   "csr_capacity"    k: (test hook, before ldp_set_variants()) the compacted rows' buffer holds k entries; a run with more non-zero words falls back
 *                     to the dense rows (0 = a quarter of all predicate words)
 *   "wide_sparse"     0/1: launches whose rows have a few missing calls keep the 8 x 8 tiles of wide-band subcontigs (the tile kernel's
 *                     SPARSE instantiation; default 1); 0 = they fall back to the parallelogram plan as in rounds 2-5
 *   "tile_route"      0/1: prune launches whose wide-band subcontigs stay on the tile plan on every route decide PER TILE, on the device and from the
 *                     records of the rows the tile multiplies, which of the three tile kernels runs it: the complete-data body, the SPARSE
 *                     instantiation or the quarter tiles, never above the launch's route word (default 1); 0 = the word sends
 *                     every tile of the launch to one kernel, as in rounds 2-6.  Any other value: LDP_ERR_INVALID
 *   "wide_diag_kernel" 0/1: complete-data prune launches run the tiles ON the diagonal (36 live products, to the end of the rows) in eight 2 x 3
 *                     rectangles, a second body of pair_mfma_wide_kernel picked per workgroup (default 1); 0 = 2 x 4 rectangles for every tile
 *   "wide_diag_corner" 0/1: where "wide_diag_kernel" applies, the diagonal tile also computes the one product of its J tile's distance-1 tile that
 *                     lies next to the block diagonal -- (J block 0, V block 7), row-block 8 t against 8 t - 1 -- in a slot of its wave 0 that is
 *                     otherwise beyond the plan, and the distance-1 tile retires with the far tiles (default 1); 0 = every tile computes its own
 *                     products.  The plan (ldp_debug_wide_plan) is the same either way
 *   "wide_diag_last"  k: within a launch every XCD's stream of 8 x 8 tiles runs its far tiles first and the tiles fewer than k tile
 *                     distances from the diagonal (the long ones: they hold the pairs in LD) at the end; 0 = plain J order (default 1: the
 *                     diagonal tiles, which with "wide_diag_corner" hold every product next to the block diagonal; 2 until then; before
 *                     ldp_set_variants())
 *   "wide_min_reach"  row-blocks a subcontig's band must reach to take the 8 x 8 tile plan of the wide-band kernel; 0 = always,
 *                     a huge value = never (before ldp_set_variants())
 *   "replay_steps"    k: ldp_debug_replay_pairs() walks every subcontig in k instalments, the way the streaming replay of a run advances
 *   "replay_csr"      0/1/2: ldp_debug_replay_pairs() builds the CSR form of its dense rows with a plain host loop -- per row (first entry, entries),
 *                     per non-zero word (word index inside the row, bits), ascending: the written specification of pred_compact_kernel's output
 *                     -- and replays through the view a production run reads; 1 = the runs of the 64-row blocks ascend, 2 = they descend (the
 *                     device's blocks land in the order of their atomic adds); 0 = the dense rows (default).  Other values: LDP_ERR_INVALID
 *   "decode_rows"     k: ldp_load_pgen_records*() decode in launches of k rows (LD chains cut everywhere)
 *   "decode_no_lds"   0/1: decoded rows are assembled in global memory (what rows beyond 128 KiB take) instead of LDS
 *   "x_rows"          k: ldp_r2_unphased_block_x*() work in chunks of k rows
 *   "compact_batch_rows" k: ldp_restrict_variants() moves the image in batches of k rows (0 = as many as 256 MiB hold): which batches
 *                     are copied directly and which go through the bounce buffer depends on rows per batch
 *   "sample_missing_slab_rows" k: ldp_sample_missing_counts() cuts its rows into slabs of k (at most 8160: 32 row lanes x the 255 an
 *                     8-bit counter field holds); 0 = full slabs on a large image, shorter ones on a small image
 * Results never depend on these.  Unknown name: LDP_ERR_INVALID. */
int ldp_debug_set_option(ldp_engine* e, const char* name, double value);
/* The .pgen reader's phase / subset routines use pext / pdep where the host has BMI2; on != 0 forces the portable loops for the whole
 * process (a test hook: both give the same bytes). */
int ldp_pgen_debug_force_portable(int on);
/* Host-only view of the matrix-pipe work plan (csrc/ldp_device.h: MfmaWG) in the engine's shard-local variant
 * indices, for the CPU test that every candidate pair is owned by exactly one 32 x 32 block product.  Per workgroup
 * 63 words: n_rb (bit 31: see ldp_debug_wide_plan; bit 30: every wave item is diagonal), j_lo, j_hi, rb[16], then per wave jv, vv, jend, prod_mask, slot[7].  lo_local (optional, *local_ct
 * entries) receives the window starts in the same index space.  words == NULL only counts. */
int ldp_debug_mfma_plan(const ldp_engine* e, uint32_t* wg_count, uint32_t* words, uint64_t capacity_words, uint32_t* lo_local, uint32_t* local_ct);

/* The wide-band plan (csrc/ldp_device.h: MfmaTile; subcontigs whose band reaches the "wide_min_reach" option in row-blocks): per
 * tile 5 words: jv, vv, jend, mask bits 0-31, mask bits 32-63 (bit 8 a + b: the product of J block a and V block b).  The
 * workgroups of ldp_debug_mfma_plan() that belong to such subcontigs carry bit 31 in their first word; complete-data launches
 * leave those to the tiles.  words == NULL only counts. */
int ldp_debug_wide_plan(const ldp_engine* e, uint32_t* tile_count, uint32_t* words, uint64_t capacity_words);

/* The wave -> rectangle map of the DIAGONAL tiles' 2 x 3 body ("wide_diag_kernel"; csrc/ldp_device.h: kWdDiagMap, the table the kernel's
 * constants are made from), no engine and no GPU needed.  Per wave (eight of them; waves w and w + 4 share a SIMD) 5 words: a0, b0 (the
 * rectangle: J blocks a0, a0 + 1 x V blocks b0 .. b0 + 2), cols (bit b: the wave owns the products of V block b0 + b), then the products
 * it owns as mask bits 0-31 / 32-63 in ldp_debug_wide_plan()'s layout (bit 8 a + b).  capacity_words < 40: LDP_ERR_INVALID. */
int ldp_debug_wide_diag_map(uint32_t* words, uint64_t capacity_words);

/* The class every tile of the last run ran on ("tile_route"), one byte per tile in the order of ldp_debug_wide_plan(): bits 0-1 the class
 * (0 complete-data body, 1 SPARSE tiles, 2 quarter tiles), bit 2: the tile -- a diagonal one -- computed the corner product of its
 * neighbour, bit 3: the tile -- one tile distance from the diagonal -- left its corner product to the diagonal tile; as the tile actually
 * ran.  LDP_ERR_STATE before a run and after a run that did not route its tiles one by one (ldp_get_tile_routes() is all zero then),
 * LDP_ERR_INVALID when capacity < tiles. */
int ldp_debug_tile_classes(ldp_engine* e, uint8_t* out, uint64_t capacity, uint32_t* tile_count);


/* What the last ldp_restrict_variants() moved: image rows in all, of them copied directly / through the bounce buffer (a row that
 * stays where it is counts nowhere), and the device time of the image's compaction (HIP events on the engine's stream).  Any
 * pointer may be NULL. */
int ldp_debug_get_compact_stats(const ldp_engine* e, uint64_t* rows_compacted, uint64_t* rows_direct, uint64_t* rows_bounced, double* ms_compact);

/* What the last ldp_sample_missing_counts() did: the device time of its kernel launches (HIP events on the engine's stream) and the bytes
 * of the image they read (rows x row pitch).  Any pointer may be NULL. */
int ldp_debug_get_sample_missing_stats(const ldp_engine* e, double* ms_kernel, uint64_t* bytes_read);

/* ldp_sample_het_counts() with its test and measurement hooks as arguments -- the call keeps no state in the engine --: slab_rows cuts the
 * rows into slabs of that many (at most 8160, as for "sample_missing_slab_rows"; 0 = chosen by the launch; results never depend on it);
 * *ms_kernel and *bytes_read (either may be NULL) receive the device time of the kernel launches (HIP events on the engine's stream) and
 * the bytes of the image they read (rows x row pitch). */
int ldp_debug_sample_het_counts(ldp_engine* e, uint32_t first_variant, uint32_t n, const uint8_t* include, const uint64_t* weight, uint32_t* het_ct, uint32_t* missing_ct,
                                uint64_t* missing_weight, uint32_t slab_rows, double* ms_kernel, uint64_t* bytes_read);

/* ldp_king_counts_block() with its test and measurement hooks as arguments -- the call keeps no state in the engine --: slab_variants
 * cuts the variants into slabs of that many (a multiple of 256, at most 65536, otherwise LDP_ERR_INVALID; 0 = chosen from the block's
 * sample counts so that the strips stay below the scratch cap; results never depend on it); *ms_kernel and *pair_variants (either may
 * be NULL) receive the device time of the launches (HIP events on the engine's stream) and the pairs of the block times the included
 * variants. */
int ldp_debug_king_counts_block(ldp_engine* e, uint32_t first_variant, uint32_t n, const uint8_t* include, uint32_t row_first, uint32_t row_ct, uint32_t col_first,
                                uint32_t col_ct, ldp_king_counts_t* out, uint64_t ld_elems, uint32_t slab_variants, double* ms_kernel, uint64_t* pair_variants);

/* ldp_hwe_ln_pvals() / ldp_hwe_ln_pvals_counts() with their measurement hook as an argument -- neither keeps state --: *ms_kernel (may be
 * NULL) receives the device time of the hwe_kernel launches (HIP events on the stream they run on). */
int ldp_debug_hwe_ln_pvals(ldp_engine* e, uint32_t first_variant, uint32_t n, int midp, double* ln_p, uint8_t* flags, double* ms_kernel);
int ldp_debug_hwe_ln_pvals_counts(int device, uint32_t n, const uint32_t* hom1, const uint32_t* het, const uint32_t* hom2, int midp, double* ln_p, uint8_t* flags,
                                  double* ms_kernel);

/* What the last ldp_r2_phased_* call on this engine did (ldp_counters has no room left for it): the pairs its device-side filter saw
 * and the pairs it dropped (both 0 for the calls that do not filter), and the device time, HIP events on the engine's stream, of the
 * double-heterozygote product kernel (ldp_pair_phased.hip) and of the six-integer pair launches of the same call, summed over its
 * chunks and over both engines when there are phase rows.  Any pointer may be NULL. */
int ldp_debug_get_phased_filter(const ldp_engine* e, uint64_t* pairs_seen, uint64_t* pairs_dropped, double* ms_hethet, double* ms_tuples);

/* The checkpoint statistics the count pass of the loads wrote for variants [first_variant, first_variant + n), as they lie on the device
 * (csrc/ldp_device.h): cp_out receives n records of 144 bytes -- nine 16-byte slots: five remainder slots and the whole-row slot
 * {double a, b}, then on a code-image engine the whole-row and two remainder slots {uint32 calls, sum z, sum z^2, flag} (left as
 * allocated on a bit-plane engine) --, cp_gen_out n rows of 80 bytes -- five {uint32 calls, sum z, sum z^2, pad}, written on bit-plane
 * engines only --, checkpoint_chunk the engine's five checkpoint chunks (0xffffffff = unused) and *n_checkpoints how many are in use.
 * Any output pointer may be NULL.  Waits for the engine's stream, then copies: no kernel is launched.  LDP_ERR_STATE before a plan is
 * on the device or for rows that are not loaded, LDP_ERR_UNSUPPORTED on a sharded engine. */
int ldp_debug_get_cp_stats(ldp_engine* e, uint32_t first_variant, uint32_t n, void* cp_out, void* cp_gen_out, uint32_t* checkpoint_chunk, uint32_t* n_checkpoints);
/* Which count kernel the last load's launch ran -- *is_codes 1 = codes_kernel (code image), 0 = prepare_kernel (bit-planes) -- and
 * the <THREADS, ITERS> instantiation the row length picked (ITERS 0 = the rolled loop).  LDP_ERR_STATE before the first load. */
int ldp_debug_get_count_pass(const ldp_engine* e, uint32_t* is_codes, uint32_t* threads, uint32_t* iters);

/* ---- synthetic workload (benchmark / test support, not part of the reference seam) ---- */
/* Deterministic genotype generator for the SURVEY.md 8(d) workload: rows [first_variant, +n_variants) of
 * REF-based codes (LDP_GENO_REF) written to `out` (host or device memory), each genotype a pure function of
 * (seed, variant index, sample index).  LD is planted like the reference's --dummy
 * (plink2_import.cc:16387-16432).  `stream` is a hipStream_t (device output only; may be NULL). */
int ldp_synth_genotypes(uint64_t seed, uint64_t first_variant, uint32_t n_variants, uint32_t founder_ct, double missing_rate,
                        void* out, uint64_t stride_bytes, int location, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LDPRUNE_HIP_DEBUG_H */
