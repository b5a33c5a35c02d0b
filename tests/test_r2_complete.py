"""The r^2 outputs of complete-data launches, every value against an independent reference.

A launch whose resident rows have no missing call at all runs pair_mfma_kernel<4, false, *> over the parallelogram plan and, once an all-pairs
request reaches 12 row-blocks, pair_mfma_wide_kernel<false> over 8 x 8 block tiles.  Their r^2 epilogue (emit_pair behind r2_out / r2_hits: row and
column clipping, dense or band index, float cast, NaN bit patterns, hit filter, six-integer tuples, signed r; the tiles' orientation fix-up and
the planner's row / column filtering before it) is compared here pair by pair -- no sampling, no tolerance, bit patterns only -- with
ldtools.band_pair_stats / band_r2 (float64 matrix products and ComputeR2's operations in numpy; tests/test_pair_reference.py checks them against
the oracle on the CPU).  Every engine asserts from the counters of the call itself which kernel ran (include/ldprune_hip.h): one missing call
anywhere would move the whole launch to the six-product kernel, and the test would prove nothing (tests/test_r2_missing.py has that kernel).
The harness -- the rows, the Reference, the Engine whose every call is compared and counted, the planner's rules, the request lists, the body of
the windowed-plan test -- lives in tests/r2_tools.py, shared with test_r2_missing.py; this file passes it the route (1, 0, 0)."""
import time

import numpy as np
import pytest

import ldtools as T
import r2_tools as R
from r2_tools import BLOCKS, CHUNKS, K_WIDE_MIN_REACH, SAMPLE_COUNTS, WINDOWS, clip, reference

pytestmark = pytest.mark.gpu

TOTALS = R.new_totals()

ENGINES = [
    ("default", {}),
    ("parallelogram", {"wide_min_reach": 1e9}),
    ("image as loaded", {"orient_rows": 0}),
]


def Engine(pkg, ref, options):
    """every call of this file must report the complete route: (route_complete_launches, route_general_launches, route_sparse_launches) = (1, 0, 0)"""
    return R.Engine(pkg, ref, options, (1, 0, 0), TOTALS)


def finish(t0, label, compared):
    R.finish(TOTALS, t0, label, compared)


@pytest.mark.parametrize("engine", ENGINES, ids=[e[0] for e in ENGINES])
@pytest.mark.parametrize("n", SAMPLE_COUNTS)
def test_matrix_rows_and_blocks(gpu_pkg, n, engine):
    """r2_unphased_rows (whole matrix in doubles, chunks in floats) and r2_unphased_block (doubles and floats) at m = 600: 19 row-blocks,
    tile rows 0, 1 and a partial 2 whose last block holds 24 rows; n below one 512-sample stage, exactly one, one sample into the second,
    three with a tail"""
    t0 = time.time()
    m = 600
    ref = reference(m, n)
    with Engine(gpu_pkg, ref, engine[1]) as e:
        got = e.rows(0, 0, m, False)
        gb = T.bits_of(got)
        il = np.tril_indices(m)
        assert set(gb[il][np.isnan(got[il])].tolist()) <= {T.R2_NAN64}
        d = gb[np.arange(m), np.arange(m)]
        novar = (ref.raw == ref.raw[:, :1]).all(1)      # complete data: no variance = one genotype throughout
        assert (d[novar] == T.R2_NAN64).all() and (d[~novar] == 0x3ff0000000000000).all() and novar.sum() >= 3
        assert not gb[np.triu_indices(m, 1)].any()
        for r0, rc in CHUNKS:
            part = e.rows(0, r0, rc, True)
            assert set(T.bits_of(part)[np.isnan(part)].tolist()) <= {T.R2_NAN32}
        for blk in BLOCKS:
            e.block(0, *blk, False)
            e.block(0, *blk, True)
        finish(t0, "rows + blocks, n = %d, %s" % (n, engine[0]), e.compared)


@pytest.mark.parametrize("engine", ENGINES, ids=[e[0] for e in ENGINES])
@pytest.mark.parametrize("n", SAMPLE_COUNTS)
def test_hit_filters_against_the_reference_list(gpu_pkg, n, engine):
    """r2_unphased_hits / _block_hits against the REFERENCE's filtered list (not the device's dense rows): thresholds 0.2, 1e-9 and 0 (every
    non-NaN pair, zeros included); pair sets equal, r^2 bit-identical, found == len; one overflow case"""
    t0 = time.time()
    ref = reference(600, n)
    with Engine(gpu_pkg, ref, engine[1]) as e:
        for thr in (0.2, 1e-9, 0.0):
            for r0, rc in CHUNKS:
                e.hits(0, thr, r0, rc)
            for blk in BLOCKS:
                e.hits(0, thr, *blk)
        f0, _, _ = ref.hits(0, 0.0, 0, 600, 0, 600)
        assert len(f0) == int((~np.isnan(ref.band[0])).sum())
        e.hits(0, 1e-9, 0, 600, capacity=10)
        e.hits(0, 0.0, 384, 216, 0, 600, capacity=10)
        finish(t0, "hits, n = %d, %s" % (n, engine[0]), e.compared)


@pytest.mark.parametrize("engine", ENGINES, ids=[e[0] for e in ENGINES])
@pytest.mark.parametrize("n", SAMPLE_COUNTS)
def test_pair_tuples_of_blocks(gpu_pkg, n, engine):
    """pair_stats_block: the six integers of every pair i < j of a block equal band_pair_stats, zero bits elsewhere"""
    t0 = time.time()
    ref = reference(600, n)
    with Engine(gpu_pkg, ref, engine[1]) as e:
        for blk in BLOCKS:
            e.tuples(*blk)
        finish(t0, "tuples, n = %d, %s" % (n, engine[0]), e.compared)


@pytest.mark.parametrize("engine", ENGINES, ids=[e[0] for e in ENGINES])
@pytest.mark.parametrize("n", [90, 513])
@pytest.mark.parametrize("mode", [1, 2])
def test_signed_r(gpu_pkg, mode, n, engine):
    """set_r_signed(1) / (2): rows, blocks and hits with |r| >= 0.3 equal +-sqrt(r^2) with the covariance's sign in the major-allele /
    the REF orientation (the latter from REF-oriented products, not from flipped flags); +0.0 at a zero covariance, NaN untouched"""
    t0 = time.time()
    m = 600
    ref = reference(m, n)
    zero = ref.band[mode] == 0.0
    assert zero.any() and not T.bits_of(ref.band[mode])[zero].any() and (ref.band[mode][~np.isnan(ref.band[mode])] < 0).any()
    if mode == 2:
        assert (np.signbit(ref.band[2]) != np.signbit(ref.band[1])).sum() > 1000
    with Engine(gpu_pkg, ref, engine[1]) as e:
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
        finish(t0, "signed r mode %d, n = %d, %s" % (mode, n, engine[0]), e.compared)


@pytest.mark.parametrize("m,min_reach", [(384, None), (385, None), (200, 0)])
def test_the_counters_flip_where_the_planner_takes_tiles(gpu_pkg, m, min_reach):
    """m = 384: reach 11, no tile; m = 385: reach 12, tiles with a one-row last block; m = 200 with wide_min_reach 0: one partial tile.
    Rows, blocks, hits and tuples at each, on the three engines."""
    t0 = time.time()
    n = 90
    ref = reference(m, n)
    total = 0
    for label, options in ENGINES:
        if min_reach is not None and "wide_min_reach" not in options:
            options = dict(options, wide_min_reach=min_reach)
        with Engine(gpu_pkg, ref, options) as e:
            e.rows(0, 0, m, False)
            c = e.eng.counters()
            want_tiles = (m == 385 or min_reach == 0) and options.get("wide_min_reach", K_WIDE_MIN_REACH) < 1e9
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
    finish(t0, "m = %d, wide_min_reach %s" % (m, min_reach), total)


@pytest.mark.parametrize("bp_radius,var_radius", WINDOWS)
@pytest.mark.parametrize("n", [90, 1100])
def test_windowed_plan(gpu_pkg, n, bp_radius, var_radius):
    """set_variants_vcor over chromosome runs [250, 1, 349]: launches without tiles, pair_mfma_kernel<4, false, diag> and its general-form
    sibling -- whole-chromosome windows (reach up to 10 blocks, several wave items per block pair), 40 variants, and a narrow bp window.
    band()'s lo against UpdateVcorWindow's rule; band rows whole and in chunks, doubles and floats; hits with global indices."""
    t0 = time.time()
    ref = reference(600, n)
    cand, compared = R.windowed_plan_case(gpu_pkg, ref, bp_radius, var_radius, {}, (1, 0, 0), TOTALS)
    finish(t0, "windowed plan n = %d, window (%d, %d): %d candidate pairs" % (n, bp_radius, var_radius, cand), compared)


def test_zz_totals():
    print("pairs compared in this file: %d over %d counted calls, %.1f s in its tests" % (TOTALS["compared"], TOTALS["calls"], TOTALS["seconds"]))
    assert TOTALS["compared"] > 0 and TOTALS["calls"] > 0
