"""Every candidate pair's prune decision, on the kernels production runs.

ldp_run() leaves the dense predicate rows in device memory; ldp_debug_get_pred() (LdPruneEngine.last_pred) hands them out.  Each case
here runs an engine with the PRODUCTION settings (early termination on, the route decided per launch group, interval epilogues, tiles)
plus the case's options, and compares the decision of EVERY candidate pair -- no sampling, no tolerance -- with an independent float64
reference (ldtools.band_pair_stats / band_decisions: matrix products and three multiplications, checked against the oracle on the CPU in
tests/test_pair_reference.py):
  (a) last_pred() == reference for all pairs (a mismatch names the pairs, their integers and cov^2 / (thr var1 var2));
  (b) last_pred().sum() == counters()["pred_true"]: every pair owned and counted once;
  (c) no bit outside the band;
  (d) the prune set equals the oracle's;
  (e) the counters prove that the intended kernel ran.
The prune set alone hides most single wrong decisions, and the inspection run (run_with_stats) switches the checkpoints,
the interval epilogues and the per-group routes off: neither sees what these cases see."""
import numpy as np
import pytest

import ldtools as T
from test_host_logic import make_positions
from test_gpu_parity import (RUN_CASES, WIDE_CASES, SPARSE_WIDE_CASES, FEW_MISSING_CASES, FOUR_PRODUCT_CASES, QUARTER_TILE_CASES, wide_rows,
                             sparse_wide_rows, few_missing_rows, four_product_rows, quarter_tile_rows)

pytestmark = pytest.mark.gpu

TOTALS = {"compared": 0, "candidate_pairs": 0, "engines": 0}


class Reference:
    """the rows of one case and what every engine over them must give: computed once per case, not per option set.
    raw_for_stats: the image's columns as REF-based codes where they are not the rows that are loaded (haplotype columns of phased rows,
    gathered columns of sample-mapped rows, the REF-coded form of INVERSE rows): the statistics, the founder count and -- unless `removed`
    is given -- the prune set come from them.  removed: the prune set, where another oracle computes it (--indep-pairphase, host-built rows)."""

    def __init__(self, pkg, raw, chr_idx, bps, window, step, is_bp, r2, order, raw_for_stats=None, removed=None):
        self.raw, self.chr_idx, self.bps = raw, np.asarray(chr_idx, dtype=np.uint32), bps
        self.window, self.step, self.is_bp, self.r2, self.order = window, step, is_bp, r2, order
        self.raw_for_stats = raw if raw_for_stats is None else raw_for_stats
        self.m, self.n = self.raw_for_stats.shape
        assert raw.shape[0] == self.m
        self.packed = T.pack_2bit(raw)
        eng = pkg.LdPruneEngine(self.n, window, step, is_bp, r2, order=order, device=0)
        eng.set_variants(self.chr_idx, bps)
        self.lo, self.cand = eng.band()
        eng.close()
        self.stats = T.band_pair_stats(self.raw_for_stats, self.lo)
        assert len(self.stats) == self.cand
        self.dec = T.band_decisions(self.stats, r2)
        if removed is None:
            inv, mf, _ = T.oracle_prepare(self.raw_for_stats)
            removed, _ = T.oracle_indep_pairwise(inv, self.n, self.chr_idx, bps if bps is not None else np.arange(self.m, dtype=np.uint32), mf, window,
                                                 step, is_bp, r2, order)
        self.removed = removed


def run_and_compare(pkg, eng, ref, options, expect=None, label="", totals=None):
    """one production run of a loaded engine; (a)-(e); returns the counters"""
    totals = TOTALS if totals is None else totals
    removed = eng.run()
    pred, outside = eng.last_pred(with_outside=True)
    c = eng.counters()
    totals["compared"] += len(pred)
    totals["candidate_pairs"] += c["candidate_pairs"]
    totals["engines"] += 1
    print("pairs compared: %d  (%s %s; %d true; launches %d, routes complete/sparse/general %d/%d/%d, sparse/four tile launches %d/%d, skipped product stages %d)"
          % (len(pred), label, options, int(pred.sum()), c["pair_kernel_launches"], c["route_complete_launches"], c["route_sparse_launches"],
             c["route_general_launches"], c["sparse_tile_launches"], c["four_tile_launches"], c["mfma_skipped_product_stages"]))
    assert c["candidate_pairs"] == ref.cand == len(pred)
    nd, msg = T.compare_decisions(pred, ref.dec, ref.lo, ref.stats, ref.r2, counters=c)
    assert nd == 0, "%s %s\n%s" % (label, options, msg)                                      # (a)
    assert int(pred.sum()) == c["pred_true"], (label, options, int(pred.sum()), c["pred_true"])   # (b)
    assert outside == 0, (label, options, "bits set outside the band", outside)            # (c)
    assert np.array_equal(removed, ref.removed), (label, options, int(removed.sum()), int(ref.removed.sum()))   # (d)
    if expect is not None:
        expect(c)                                                                            # (e)
    return c


def decide(pkg, ref, options, expect=None, loads=None, label="", load=None, inspect=None, totals=None):
    """one production run over ref's rows with `options`; (a)-(e); returns the counters.
    load: a callable (pkg, eng, ref) that brings the rows into the planned engine instead of ldp_load_genotypes() from host memory (it may
    plan the engine again, set a sample map or frequencies -- whatever its input form takes).  inspect: a callable (eng, counters) run
    after the comparison, before the engine is closed."""
    eng = pkg.LdPruneEngine(ref.n, ref.window, ref.step, ref.is_bp, ref.r2, order=ref.order, device=0)
    try:
        for name, value in options.items():
            eng.set_option(name, value)
        eng.set_variants(ref.chr_idx, ref.bps)
        if load is not None:
            load(pkg, eng, ref)
        else:
            for a, b in (loads or [(0, ref.m)]):
                eng.load_genotypes_host(a, ref.packed[a:b], pkg.LDP_GENO_REF)
        c = run_and_compare(pkg, eng, ref, options, expect, label, totals)
        if inspect is not None:
            inspect(eng, c)
    finally:
        eng.close()
    return c


# ---------------------------------------------------------------- the hook itself
def test_the_hook_returns_what_the_inspection_run_decided(gpu_pkg):
    """Self-check of ldp_debug_get_pred: after run_with_stats() the predicate rows must be band_decisions() of the device's own tuples (which
    tests/test_gpu_parity.py compares with the oracle one by one) -- order, masking and bit layout of the hook.  Then its refusals."""
    pkg = gpu_pkg
    for case, min_reach in ((RUN_CASES[2], None), (RUN_CASES[4], None), (WIDE_CASES[1], 12)):
        m, n, seed, window, step, is_bp, r2, order = case[:8]
        raw = T.synth_raw_codes(m, n, seed, missing_rate=0.04)
        chr_idx, bps = make_positions(m, 3, seed + 100)
        eng = pkg.LdPruneEngine(n, window, step, is_bp, r2, order=order, device=0)
        if min_reach is not None:
            eng.set_option("wide_min_reach", min_reach)
        eng.set_variants(chr_idx, bps)
        with pytest.raises(pkg.LdpError) as ei:
            eng.last_pred()                                   # nothing loaded, nothing run
        assert ei.value.code == pkg.LDP_ERR_STATE
        eng.load_genotypes_host(0, T.pack_2bit(raw), pkg.LDP_GENO_REF)
        with pytest.raises(pkg.LdpError) as ei:
            eng.last_pred()                                   # loaded, not run
        assert ei.value.code == pkg.LDP_ERR_STATE
        removed, stats = eng.run_with_stats()
        pred, outside = eng.last_pred(with_outside=True)
        lo, cand = eng.band()
        want = T.band_decisions(stats, r2)
        nd, msg = T.compare_decisions(pred, want, lo, stats, r2, counters=eng.counters())
        assert nd == 0, msg
        assert outside == 0 and int(pred.sum()) == eng.counters()["pred_true"] > 0
        # ... and the independent reference agrees with the device's tuples
        assert np.array_equal(T.band_pair_stats(raw, lo), np.stack([stats[f].astype(np.int64) for f in T.PAIR_FIELDS], 1))
        # the production run on the same engine: the same decisions
        assert np.array_equal(eng.run(), removed)
        assert np.array_equal(eng.last_pred(), pred)
        TOTALS["compared"] += 2 * cand
        TOTALS["candidate_pairs"] += 2 * cand
        print("pairs compared: %d (inspection run) + %d (production run)" % (cand, cand))
        # a short buffer is refused; a load invalidates the rows (they are cleared as launches are queued)
        import ctypes
        buf = np.zeros(max(cand, 1), dtype=np.uint8)
        assert pkg.lib().ldp_debug_get_pred(eng._h, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), cand - 1, None) == pkg.LDP_ERR_INVALID
        eng.load_genotypes_host(0, T.pack_2bit(raw[:5]), pkg.LDP_GENO_REF)
        with pytest.raises(pkg.LdpError) as ei:
            eng.last_pred()
        assert ei.value.code == pkg.LDP_ERR_STATE
        eng.close()
    # sharded engines are refused
    eng = pkg.LdPruneEngine(n, window, step, is_bp, r2, order=order, device=0)
    eng.set_variants(chr_idx, bps)
    eng.set_shard(0, 2)
    eng.load_genotypes_host(0, T.pack_2bit(raw), pkg.LDP_GENO_REF)
    eng.run()
    with pytest.raises(pkg.LdpError) as ei:
        eng.last_pred()
    assert ei.value.code == pkg.LDP_ERR_UNSUPPORTED
    eng.close()


# ---------------------------------------------------------------- complete data
def _complete_route(c):
    assert c["route_complete_launches"] > 0 and c["route_sparse_launches"] == 0 and c["route_general_launches"] == 0


@pytest.mark.parametrize("case", [c for c in RUN_CASES if c[8] == 0.0])
def test_complete_rows_parallelogram_plan(gpu_pkg, case):
    m, n, seed, window, step, is_bp, r2, order, miss = case
    raw = T.synth_raw_codes(m, n, seed, missing_rate=0.0)
    chr_idx, bps = make_positions(m, 3, seed + 100)
    ref = Reference(gpu_pkg, raw, chr_idx, bps, window, step, is_bp, r2, order)

    def expect(c):
        _complete_route(c)
        assert c["wide_tiles"] == 0 and c["mfma_block_products"] > 0
    decide(gpu_pkg, ref, {"wide_min_reach": 1e9}, expect, label="complete/parallelogram")
    decide(gpu_pkg, ref, {}, _complete_route, label="complete/default plan")


@pytest.mark.parametrize("n,r2", [(20000, 0.5), (20000, 0.05)])
def test_complete_rows_parallelogram_plan_with_checkpoints(gpu_pkg, n, r2):
    """40 stages of 512 samples: at r^2 0.5 the checkpoints retire products (asserted), at 0.05 hardly any pair is hopeless early"""
    m = 700
    raw = T.synth_raw_codes(m, n, seed=n % 97, missing_rate=0.0)
    chr_idx, bps = make_positions(m, 2, 5)
    ref = Reference(gpu_pkg, raw, chr_idx, bps, 150, 1, False, r2, 2)

    def expect(c):
        _complete_route(c)
        assert c["wide_tiles"] == 0
        if r2 >= 0.5:
            assert c["mfma_skipped_product_stages"] > 0
    decide(gpu_pkg, ref, {"wide_min_reach": 1e9}, expect, label="complete/parallelogram/checkpoints")


def _wide_complete(c):
    _complete_route(c)
    assert c["wide_tiles"] > 0


@pytest.mark.parametrize("case", WIDE_CASES)
def test_complete_rows_on_the_tiles(gpu_pkg, case):
    """pair_mfma_wide_kernel: 8 x 8 tiles, the diagonal ones in 2 x 3 rectangles ("wide_diag_kernel" 1, the default) or in the 2 x 4
    rectangles of every other tile (0).  Wide-plan engines have ONE launch group by design (kTargetGroups = 1 when the tiles hold most
    products), so two routes in one run cannot occur here."""
    m, n, seed, window, step, is_bp, r2, order, min_reach = case
    raw, chr_idx, bps = wide_rows(case)
    ref = Reference(gpu_pkg, raw, chr_idx, bps, window, step, is_bp, r2, order)
    for dk in (1, 0):
        decide(gpu_pkg, ref, {"wide_min_reach": min_reach, "wide_diag_kernel": dk}, _wide_complete, label="complete/tiles")


def test_complete_rows_on_the_tiles_with_checkpoints(gpu_pkg):
    """n = 20,000: 40 stages, so the tiles' checkpoints retire products (asserted) -- with pairs that only become correlated in the last
    40 % of the samples, 37 rows (another row-block) apart"""
    m, n, window, r2 = 1500, 20000, 600, 0.5
    rng = np.random.default_rng(n + m)
    raw = T.synth_raw_codes(m, n, 11, missing_rate=0.0, ld_copy_prob=0.6, redraw=0.08)
    cut = int(0.6 * n)
    for v in range(40, m, 11):
        raw[v, :cut] = rng.permutation(raw[v, :cut])
        raw[v, cut:] = raw[v - 37, cut:]
    chr_idx = np.repeat(np.arange(2, dtype=np.uint32), m // 2)
    ref = Reference(gpu_pkg, raw, chr_idx, None, window, 1, False, r2, 2)

    def expect(c):
        _wide_complete(c)
        assert c["mfma_skipped_product_stages"] > 0
    for dk in (1, 0):
        decide(gpu_pkg, ref, {"wide_min_reach": 12, "wide_diag_kernel": dk}, expect, label="complete/tiles/checkpoints")


# ---------------------------------------------------------------- a few missing calls: the interval epilogues
def _sparse_route(c):
    assert c["route_sparse_launches"] > 0 and c["route_general_launches"] == 0 and c["route_complete_launches"] == 0


@pytest.mark.parametrize("n,miss,r2,redraw,frac", FEW_MISSING_CASES)
def test_a_few_missing_calls_parallelogram_plan(gpu_pkg, n, miss, r2, redraw, frac):
    """sparse_round / sparse_decide: intervals settle most pairs, the rest is recounted"""
    raw, chr_idx, bps = few_missing_rows(n, miss, redraw)
    ref = Reference(gpu_pkg, raw, chr_idx, bps, 150, 1, False, r2, 2)

    def expect(c):
        _sparse_route(c)
        assert c["sparse_tile_launches"] == 0 and c["wide_tiles"] == 0
    decide(gpu_pkg, ref, {} if frac is None else {"sparse_frac": frac}, expect, label="few missing/parallelogram")


@pytest.mark.parametrize("case", SPARSE_WIDE_CASES)
def test_a_few_missing_calls_on_the_tiles(gpu_pkg, case):
    """pair_mfma_wide_kernel<SPARSE> (classify_sparse): late LD 37 rows back, rare variants whose partners miss calls on the carriers,
    complete rows, rows at 7 % missing"""
    m, n, window, step, is_bp, r2, order, min_reach, miss, adversarial = case
    raw, chr_idx, bps = sparse_wide_rows(case)
    ref = Reference(gpu_pkg, raw, chr_idx, bps, window, step, is_bp, r2, order)

    def expect(c):
        _sparse_route(c)
        assert c["wide_tiles"] > 0 and c["sparse_tile_launches"] > 0
        if (n >= 9000) and not adversarial:
            assert c["mfma_skipped_product_stages"] > 0
    decide(gpu_pkg, ref, {"wide_min_reach": min_reach}, expect, label="few missing/tiles")


# ---------------------------------------------------------------- many missing calls: four and six products
def _general_route(c):
    assert c["route_general_launches"] > 0 and c["route_sparse_launches"] == 0 and c["route_complete_launches"] == 0


@pytest.mark.parametrize("n,miss,r2,redraw", FOUR_PRODUCT_CASES)
def test_four_products_parallelogram_plan(gpu_pkg, n, miss, r2, redraw):
    """classify_four over the parallelogram plan, both operand sets ("pair_gu" 1 / 0), checkpoints on"""
    raw, chr_idx, bps = four_product_rows(n, miss, redraw)
    ref = Reference(gpu_pkg, raw, chr_idx, bps, 150, 1, False, r2, 2)

    def expect(c):
        _general_route(c)
        assert c["four_tile_launches"] == 0
    cs = [decide(gpu_pkg, ref, opts, expect, label="four products/parallelogram") for opts in ({"pair_sparse": 0}, {"pair_sparse": 0, "pair_gu": 0})]
    assert cs[0]["mfma_skipped_product_stages"] == cs[1]["mfma_skipped_product_stages"]
    if (n, miss, r2) == (20000, 0.01, 0.5):
        # six products with checkpoints (pair_hopeless over all six accumulators)
        def expect6(c):
            _general_route(c)
            assert c["sparse_exact_pairs"] == 0 and c["mfma_skipped_product_stages"] > 0
        decide(gpu_pkg, ref, {"pair_sparse": 0, "pair_four": 0}, expect6, label="six products/parallelogram/checkpoints")


@pytest.mark.parametrize("n,m,window,miss,r2", QUARTER_TILE_CASES)
def test_four_products_on_quarter_tiles(gpu_pkg, n, m, window, miss, r2):
    """pair_mfma_tile4_kernel, both operand sets, checkpoints on (n up to 50,000)"""
    raw, chr_idx = quarter_tile_rows(n, m, miss)
    ref = Reference(gpu_pkg, raw, chr_idx, None, window, 1, False, r2, 2)

    def expect(c):
        _general_route(c)
        assert c["wide_tiles"] > 0 and c["four_tile_launches"] > 0
        if n >= 6000:
            assert c["mfma_skipped_product_stages"] > 0
    for opts in ({"pair_sparse": 0}, {"pair_sparse": 0, "pair_gu": 0}):
        decide(gpu_pkg, ref, opts, expect, label="four products/quarter tiles")
    if (n, m) == (20000, 1500):
        def expect6(c):
            _general_route(c)
            assert c["four_tile_launches"] == 0 and c["sparse_exact_pairs"] == 0
        decide(gpu_pkg, ref, {"pair_sparse": 0, "pair_four": 0}, expect6, label="six products/wide band/checkpoints")


# ---------------------------------------------------------------- the popcount kernels
@pytest.mark.parametrize("n,miss,r2", [(2100, 0.03, 0.5), (5000, 0.0, 0.2), (5000, 0.0, 0.9)])
def test_popcount_kernels_with_early_termination(gpu_pkg, n, miss, r2):
    """"pair_mfma" 0: bit-planes and the popcount tile kernels (what engines beyond the matrix pipe's founder limit run), early exit on"""
    m = 700
    raw = T.synth_raw_codes(m, n, seed=n % 97, missing_rate=miss)
    chr_idx, bps = make_positions(m, 2, 5)
    ref = Reference(gpu_pkg, raw, chr_idx, bps, 150, 1, False, r2, 2)

    def expect(c):
        assert c["mfma_block_products"] == 0 and c["tile_unit_chunks"] > 0
        if (r2 >= 0.9) and (miss == 0.0):   # unrelated pairs are provably hopeless after the first of five 1024-sample chunks
            assert c["early_exit_unit_chunks"] > 0
    decide(gpu_pkg, ref, {"pair_mfma": 0}, expect, label="popcount")


# ---------------------------------------------------------------- two routes in one run
def _two_group_rows(missing_rows, miss):
    """20,000 rows over two chromosomes, 700 samples; `missing_rows` (a slice) miss `miss` of their calls, the others none"""
    m, n = 20000, 700
    raw = T.synth_raw_codes(m, n, seed=2026, missing_rate=0.0, ld_copy_prob=0.6, redraw=0.1)
    rng = np.random.default_rng(int(miss * 1e6) + 1)
    part = raw[missing_rows]
    part[rng.random(part.shape) < miss] = 3
    raw[missing_rows] = part
    assert (raw[missing_rows] == 3).any()
    chr_idx = np.repeat(np.arange(2, dtype=np.uint32), m // 2)
    return raw, chr_idx


# Narrow plans have up to two launch groups of at least 512 work items (32 second variants x up to 96 distances each): 626 items here, so
# group 0 is items [0, 512) = the rows below ~16,400 and group 1 the rest.  The cut between complete and incomplete rows lies behind
# group 0's last row (need_end), at 18,000.
TWO_GROUP_CUT = 18000


@pytest.mark.parametrize("miss,second_route", [(0.001, "route_sparse_launches"), (0.05, "route_general_launches")])
def test_two_routes_in_one_run(gpu_pkg, miss, second_route):
    """The route is decided per launch group from the records of rows [0, need_end): a fileset whose last rows miss calls and whose
    early rows do not sends group 0 to the complete-data kernel and group 1 to the interval epilogue (0.1 % missing) or the four-product
    form (5 %) IN THE SAME RUN.  The inspection run routes once and cannot see this."""
    raw, chr_idx = _two_group_rows(slice(TWO_GROUP_CUT, None), miss)
    ref = Reference(gpu_pkg, raw, chr_idx, None, 80, 1, False, 0.2, 2)

    def expect(c):
        assert c["pair_kernel_launches"] >= 2
        assert c["route_complete_launches"] > 0 and c[second_route] > 0
        assert c["route_complete_launches"] + c[second_route] == c["pair_kernel_launches"]
    decide(gpu_pkg, ref, {}, expect, label="two routes")
    if miss == 0.05:
        # ... loaded in three uneven calls: group 0 is launched from inside the second one (launch_ready_groups), group 1 by run()
        decide(gpu_pkg, ref, {}, expect, loads=[(0, 7001), (7001, 17500), (17500, ref.m)], label="two routes/eager launches")


@pytest.mark.parametrize("miss,route", [(0.001, "route_sparse_launches"), (0.05, "route_general_launches")])
def test_missing_calls_in_the_first_rows_take_every_group_off_the_complete_route(gpu_pkg, miss, route):
    """The mirror image: only rows [0, 2000) miss calls.  Group 1 multiplies none of them, but its route reads the records from row 0,
    so both groups leave the complete-data kernel."""
    raw, chr_idx = _two_group_rows(slice(0, 2000), miss)
    ref = Reference(gpu_pkg, raw, chr_idx, None, 80, 1, False, 0.2, 2)

    def expect(c):
        assert c["pair_kernel_launches"] >= 2 and c["route_complete_launches"] == 0 and c[route] > 0
    decide(gpu_pkg, ref, {}, expect, label="mirror")


def test_zz_nothing_was_skipped():
    """the cases above print the number of pairs they compared; over the file it is the sum of candidate_pairs of their engines"""
    print("pairs compared in this file: %d over %d engines (sum of their candidate_pairs: %d)" % (TOTALS["compared"], TOTALS["engines"], TOTALS["candidate_pairs"]))
    assert TOTALS["compared"] == TOTALS["candidate_pairs"]
