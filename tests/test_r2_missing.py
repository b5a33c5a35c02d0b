"""The r^2 outputs of launches whose rows have missing calls, every value against an independent reference.

One code-3 genotype anywhere in the resident rows moves an r^2 launch off the complete-data kernels: queue_route(..., allow_sparse = 0, ...) writes
kRouteGeneral, the complete-data bodies and the tile kernel return at their route check, and the whole request -- the parallelogram workgroups
marked as belonging to a tile-plan subcontig included, whose tile plan is attached and stands by -- runs on pair_mfma_general_kernel<true, false>:
six products (x.x, n.n, n_i.x_j, x_i.n_j, n_i.h_j, h_i.n_j) over the joint non-missing samples and emit_pair's r^2 epilogue.  This is what the
--r2-unphased matrices, the .vcor tables, inter-chr and --clump run on real call sets.  tests/r2_tools.py has the harness of
test_r2_complete.py; the rows are r2_tools.missing_rows: per-row missing rates from none to 60 %, all-missing rows, pairs without a shared sample,
pairs whose variance vanishes on the shared samples only, missing calls on the last sample and on either side of the 512-sample stage boundary.
Compared pair by pair -- no sampling, no tolerance, bit patterns only -- with ldtools.band_pair_stats / band_r2 (tests/test_pair_reference.py
checks them against the oracle on these rows).  Every call asserts from its own counters that the general kernel ran, with the stand-by tile
plan exactly where the planner attaches one; the popcount engine (pair_mfma 0) reports zeros there and must return the same bits."""
import time

import numpy as np
import pytest

import ldtools as T
import r2_tools as R
from r2_tools import BLOCKS, CHUNKS, SAMPLE_COUNTS, WINDOWS, Engine, clip, reference_missing

pytestmark = pytest.mark.gpu

TOTALS = R.new_totals()

MATRIX_PIPE = [
    ("default", {}),
    ("parallelogram only", {"wide_min_reach": 1e9}),
    ("image as loaded", {"orient_rows": 0}),
]
ENGINES = MATRIX_PIPE + [("popcount", {"pair_mfma": 0})]
IDS = [e[0] for e in ENGINES]
SIGNED_GRID = [(mode, n) for mode in (1, 2) for n in (90, 513)]
ONE_MISSING = [(599, 512), (0, 0), (300, 255)]
PLANNER = [(384, None), (385, None), (200, 0)]
WINDOW_ENGINES = [ENGINES[0], ENGINES[3]]
CASES = 3 * len(SAMPLE_COUNTS) * len(ENGINES) + len(SIGNED_GRID) * len(ENGINES) + len(ONE_MISSING) + len(PLANNER) + len(WINDOWS) * 2 * len(WINDOW_ENGINES)


def route_of(options):
    return R.ROUTE_POPCOUNT if options.get("pair_mfma", 1) == 0 else R.ROUTE_GENERAL


def engine(pkg, ref, options):
    return Engine(pkg, ref, options, route_of(options), TOTALS)


def novariance(raw):
    """rows whose calls are all one genotype, or that have none (from the codes alone)"""
    out = np.zeros(len(raw), dtype=bool)
    for v, row in enumerate(raw):
        out[v] = len(np.unique(row[row != 3])) <= 1
    return out


@pytest.mark.parametrize("engine_", ENGINES, ids=IDS)
@pytest.mark.parametrize("n", SAMPLE_COUNTS)
def test_matrix_rows_and_blocks(gpu_pkg, n, engine_):
    """r2_unphased_rows (whole matrix in doubles, chunks in floats) and r2_unphased_block (doubles and floats) at m = 600: 19 row-blocks, the
    last of 24 rows (clipped at n_local), a stand-by tile plan of tile rows 0, 1 and a partial 2; n below one 512-sample stage, exactly one,
    one sample into the second, three with a tail"""
    t0 = time.time()
    m = 600
    ref = reference_missing(m, n)
    with engine(gpu_pkg, ref, engine_[1]) as e:
        got = e.rows(0, 0, m, False)
        gb = T.bits_of(got)
        il = np.tril_indices(m)
        assert set(gb[il][np.isnan(got[il])].tolist()) <= {T.R2_NAN64}
        d = gb[np.arange(m), np.arange(m)]
        novar = novariance(ref.raw)                      # monomorphic over its calls, or without a call
        assert (d[novar] == T.R2_NAN64).all() and (d[~novar] == 0x3ff0000000000000).all() and novar.sum() >= 3 + 3
        assert np.array_equal(d, T.bits_of(ref.diag))
        assert not gb[np.triu_indices(m, 1)].any()
        for r0, rc in CHUNKS:
            part = e.rows(0, r0, rc, True)
            assert set(T.bits_of(part)[np.isnan(part)].tolist()) <= {T.R2_NAN32}
        for blk in BLOCKS:
            e.block(0, *blk, False)
            e.block(0, *blk, True)
        R.finish(TOTALS, t0, "rows + blocks, n = %d, %s" % (n, engine_[0]), e.compared)


@pytest.mark.parametrize("engine_", ENGINES, ids=IDS)
@pytest.mark.parametrize("n", SAMPLE_COUNTS)
def test_hit_filters_against_the_reference_list(gpu_pkg, n, engine_):
    """r2_unphased_hits / _block_hits against the REFERENCE's filtered list (not the device's dense rows): thresholds 0.2, 1e-9 and 0 (every
    non-NaN pair, zeros included; no pair with nm == 0 or without variance over its shared samples); pair sets equal, r^2 bit-identical,
    found == len; two overflow cases"""
    t0 = time.time()
    ref = reference_missing(600, n)
    with engine(gpu_pkg, ref, engine_[1]) as e:
        for thr in (0.2, 1e-9, 0.0):
            for r0, rc in CHUNKS:
                e.hits(0, thr, r0, rc)
            for blk in BLOCKS:
                e.hits(0, thr, *blk)
        f0, _, _ = ref.hits(0, 0.0, 0, 600, 0, 600)
        assert len(f0) == int((~np.isnan(ref.band[0])).sum())
        e.hits(0, 1e-9, 0, 600, capacity=10)
        e.hits(0, 0.0, 384, 216, 0, 600, capacity=10)
        R.finish(TOTALS, t0, "hits, n = %d, %s" % (n, engine_[0]), e.compared)


@pytest.mark.parametrize("engine_", ENGINES, ids=IDS)
@pytest.mark.parametrize("n", SAMPLE_COUNTS)
def test_pair_tuples_of_blocks(gpu_pkg, n, engine_):
    """pair_stats_block: the six integers of every pair i < j of a block -- nm, sums and sums of squares over the joint non-missing samples,
    each row in the orientation its own calls decide -- equal band_pair_stats, zero bits elsewhere"""
    t0 = time.time()
    ref = reference_missing(600, n)
    with engine(gpu_pkg, ref, engine_[1]) as e:
        for blk in BLOCKS:
            e.tuples(*blk)
        R.finish(TOTALS, t0, "tuples, n = %d, %s" % (n, engine_[0]), e.compared)


@pytest.mark.parametrize("engine_", ENGINES, ids=IDS)
@pytest.mark.parametrize("mode,n", SIGNED_GRID)
def test_signed_r(gpu_pkg, mode, n, engine_):
    """set_r_signed(1) / (2): rows, blocks and hits with |r| >= 0.3 equal +-sqrt(r^2) with the covariance's sign in the major-allele /
    the REF orientation (the latter from REF-oriented products, not from flipped flags); +0.0 at a zero covariance, NaN untouched"""
    t0 = time.time()
    m = 600
    ref = reference_missing(m, n)
    zero = ref.band[mode] == 0.0
    assert zero.any() and not T.bits_of(ref.band[mode])[zero].any() and (ref.band[mode][~np.isnan(ref.band[mode])] < 0).any()
    assert (np.signbit(ref.band[2]) != np.signbit(ref.band[1])).sum() > 1000
    as_ref = np.where(ref.raw == 3, 0, ref.raw)          # the missing samples counted as hom-REF: another major allele for some rows
    assert (R.alt_major(ref.raw) != R.alt_major(as_ref)).any()
    with engine(gpu_pkg, ref, engine_[1]) as e:
        e.eng.set_r_signed(mode)
        e.rows(mode, 0, m, False)
        e.rows(mode, 257, 100, True)
        for blk in ((300, 300, 0, 300), (400, 150, 390, 100), (512, 88, 256, 256)):
            e.block(mode, *blk, False)
            e.block(mode, *blk, True)
        e.hits(mode, 0.3, 0, m)
        e.hits(mode, 0.3, 384, 216)
        e.hits(mode, 0.3, 300, 300, 0, 300)
        e.hits(mode, 0.0, 257, 100, 31, 200)
        e.eng.set_r_signed(0)
        e.block(0, 300, 300, 0, 300, False)
        R.finish(TOTALS, t0, "signed r mode %d, n = %d, %s" % (mode, n, engine_[0]), e.compared)


@pytest.mark.parametrize("row,sample", ONE_MISSING)
def test_one_missing_call_moves_the_whole_launch(gpu_pkg, row, sample):
    """complete_rows(600, 513) with exactly ONE code 3 -- in the last row's last sample (the one sample of the second stage), in the first
    row's first, in the middle: the counters say (0, 1, 0) on the three matrix-pipe engines, with the stand-by tile plan, and the whole matrix,
    the blocks, the tuples and the hits at 0.0 are the reference's of those rows; the unmodified rows still run the complete route"""
    t0 = time.time()
    m, n = 600, 513
    ref = R.reference_one_missing(m, n, row, sample)
    total = 0
    for label, options in MATRIX_PIPE:
        with Engine(gpu_pkg, ref, options, R.ROUTE_GENERAL, TOTALS) as e:
            e.rows(0, 0, m, False)
            c = e.eng.counters()
            assert (c["route_complete_launches"], c["route_general_launches"], c["route_sparse_launches"]) == (0, 1, 0), (label, c)
            for blk in BLOCKS:
                e.block(0, *blk, False)
                e.block(0, *blk, True)
                e.tuples(*blk)
                e.hits(0, 0.0, *blk)
            e.hits(0, 0.0, 0, m)
            total += e.compared
    with Engine(gpu_pkg, R.reference(m, n), {}, R.ROUTE_COMPLETE, TOTALS) as e:
        e.rows(0, 0, m, False)
        c = e.eng.counters()
        assert (c["route_complete_launches"], c["route_general_launches"], c["route_sparse_launches"]) == (1, 0, 0), c
        total += e.compared
    R.finish(TOTALS, t0, "one missing call at (row %d, sample %d)" % (row, sample), total)


@pytest.mark.parametrize("m,min_reach", PLANNER)
def test_where_the_planner_attaches_tiles(gpu_pkg, m, min_reach):
    """m = 384: reach 11, no tile plan; m = 385: reach 12, a stand-by plan and a one-row last block; m = 200 with wide_min_reach 0: one partial
    tile standing by.  The general kernel clips the last block at n_local either way.  Rows, chunks, blocks, hits and tuples at each, on
    every engine."""
    t0 = time.time()
    n = 90
    ref = reference_missing(m, n)
    total = 0
    for label, options in ENGINES:
        if min_reach is not None and "wide_min_reach" not in options:
            options = dict(options, wide_min_reach=min_reach)
        with engine(gpu_pkg, ref, options) as e:
            e.rows(0, 0, m, False)
            c = e.eng.counters()
            want_tiles = (m == 385 or min_reach == 0) and options.get("wide_min_reach", R.K_WIDE_MIN_REACH) < 1e9 and route_of(options) != R.ROUTE_POPCOUNT
            assert (c["wide_tiles"] > 0) == want_tiles, (m, options, c["wide_tiles"])
            if m == 200 and want_tiles:
                assert c["wide_tiles"] == 1
            for r0, rc in [clip(s, m) for s in CHUNKS] + [(m - 1, 1)]:
                e.rows(0, r0, rc, True)
                e.hits(0, 0.2, r0, rc)
                e.hits(0, 0.0, r0, rc)
            for blk in [clip(s, m) for s in BLOCKS] + [(m - 1, 1, 0, m - 1)]:
                e.block(0, *blk, False)
                e.block(0, *blk, True)
                e.hits(0, 1e-9, *blk)
                e.tuples(*blk)
            total += e.compared
    R.finish(TOTALS, t0, "m = %d, wide_min_reach %s" % (m, min_reach), total)


@pytest.mark.parametrize("engine_", WINDOW_ENGINES, ids=[e[0] for e in WINDOW_ENGINES])
@pytest.mark.parametrize("bp_radius,var_radius", WINDOWS)
@pytest.mark.parametrize("n", [90, 1100])
def test_windowed_plan(gpu_pkg, n, bp_radius, var_radius, engine_):
    """set_variants_vcor over chromosome runs [250, 1, 349] (one of them holds an all-missing row, one a complementary pair): launches without
    tiles on the general kernel's windowed form, and on the popcount kernels.  band()'s lo against UpdateVcorWindow's rule; band rows whole
    and in chunks, doubles and floats; hits with global indices."""
    t0 = time.time()
    ref = reference_missing(600, n)
    cand, compared = R.windowed_plan_case(gpu_pkg, ref, bp_radius, var_radius, engine_[1], route_of(engine_[1]), TOTALS)
    R.finish(TOTALS, t0, "windowed plan n = %d, window (%d, %d), %s: %d candidate pairs" % (n, bp_radius, var_radius, engine_[0], cand), compared)


def test_zz_totals():
    print("pairs compared in this file: %d over %d counted calls, %d cases, %.1f s in its tests" % (TOTALS["compared"], TOTALS["calls"], TOTALS["cases"], TOTALS["seconds"]))
    assert TOTALS["compared"] > 0 and TOTALS["calls"] > 0
    assert TOTALS["cases"] == CASES, "a parametrised case did not run to its end (skipped, failed or deselected): %d of %d" % (TOTALS["cases"], CASES)
