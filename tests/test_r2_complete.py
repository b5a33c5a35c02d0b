"""The r^2 outputs of complete-data launches, every value against an independent reference.

A launch whose resident rows have no missing call at all runs pair_mfma_kernel<4, false, *> over the parallelogram plan and, once an all-pairs
request reaches 12 row-blocks, pair_mfma_wide_kernel<0> over 8 x 8 block tiles.  Their r^2 epilogue (emit_pair behind r2_out / r2_hits: row and
column clipping, dense or band index, float cast, NaN bit patterns, hit filter, six-integer tuples, signed r; the tiles' orientation fix-up and
the planner's row / column filtering before it) is compared here pair by pair -- no sampling, no tolerance, bit patterns only -- with
ldtools.band_pair_stats / band_r2 (float64 matrix products and ComputeR2's operations in numpy; tests/test_pair_reference.py checks them against
the oracle on the CPU).  Every engine asserts from the counters of the call itself which kernel ran (include/ldprune_hip.h): one missing call
anywhere would move the whole launch to the six-product kernel, and the test would prove nothing."""
import time

import numpy as np
import pytest

import ldtools as T

pytestmark = pytest.mark.gpu

TOTALS = {"compared": 0, "calls": 0, "seconds": 0.0}
K_WIDE_MIN_REACH = 12      # row-blocks of 32 (kWdMinReach): the all-pairs plan takes tiles when the last requested row's block index reaches it

ENGINES = [
    ("default", {}),
    ("parallelogram", {"wide_min_reach": 1e9}),
    ("image as loaded", {"orient_rows": 0}),
]


def complete_rows(m, n, seed=7):
    """No missing call anywhere.  The generator's rows plus: late copies 37 rows back and a family of noisy copies of one row (LD across row-blocks
    and tiles, in both orientations), hom-REF / hom-ALT / all-het
    rows, an exact REF = ALT tie (n even), strongly ALT-major rows in the first tile, across the 256 / 257 tile boundary and in the last,
    partial row-block."""
    rng = np.random.default_rng(seed + 1000 * m + n)
    raw = T.synth_raw_codes(m, n, seed, missing_rate=0.0, ld_copy_prob=0.6, redraw=0.1)
    for v in range(43, m, 7):
        raw[v] = np.where(rng.random(n) < 0.15, rng.integers(0, 3, size=n), raw[v - 37])
    template = (rng.random(n) < 0.4).astype(np.uint8) + (rng.random(n) < 0.4).astype(np.uint8)
    for v in range(40, m, 5):                         # one family over the whole matrix: LD at every block distance, half of it REF / ALT swapped
        row = np.where(rng.random(n) < rng.uniform(0.05, 0.25), rng.integers(0, 3, size=n), template)
        raw[v] = 2 - row if rng.random() < 0.5 else row
    for base in range(3, m - 30, 60):                 # (three kinds per 60 rows: NaN rows in every tile row, enough of them at m = 200)
        raw[base] = 0                                 # monomorphic hom-REF
        raw[base + 6] = 2                             # monomorphic hom-ALT
        raw[base + 11] = 1                            # all het
    raw[26] = 0
    raw[26, : n // 2] = 2                             # ref_ct == alt_ct when n is even: the tie goes to REF
    for v in (5, 12, 30, 255, 256, 257, m - 20, m - 2, m - 1):
        if 0 <= v < m:
            raw[v] = np.where(rng.random(n) < 0.8, 2, rng.integers(0, 2, size=n))
    assert not (raw == 3).any()
    return raw


class Reference:
    """one fixture and everything the engines over it must return: computed once per (m, n), never changed"""

    def __init__(self, m, n):
        self.m, self.n = m, n
        self.raw = complete_rows(m, n)
        self.raw.setflags(write=False)
        self.packed = T.pack_2bit(self.raw)
        self.lo = np.zeros(m, dtype=np.int64)
        self.first, self.second = T.band_pairs(self.lo)
        self.stats = T.band_pair_stats(self.raw, self.lo)
        self.diag = T.self_r2(self.raw)
        self.band = {0: T.band_r2(self.stats), 1: T.band_r2(self.stats, signed=1),
                     2: T.band_r2(T.band_pair_stats(self.raw, self.lo, orient=False), signed=1)}
        self.full = {k: T.band_to_dense(v, self.lo, 0, m, 0, m, diag=self.diag) for k, v in self.band.items()}
        self.full32 = {k: T.r2_to_float32(v) for k, v in self.full.items()}
        for k in self.full32:                         # (the cast turns the upper triangle's zeros into zeros)
            assert not T.bits_of(self.full32[k])[np.triu_indices(m, 1)].any()
        tup = np.zeros(len(self.stats), dtype=[(f, np.int64) for f in T.PAIR_FIELDS])
        for f, name in enumerate(T.PAIR_FIELDS):
            tup[name] = self.stats[:, f]
        self.full_stats = T.band_to_dense(tup, self.lo, 0, m, 0, m)
        for a in list(self.band.values()) + list(self.full.values()) + list(self.full32.values()) + [self.stats, self.full_stats]:
            a.setflags(write=False)
        self.input_conditions()

    def input_conditions(self):
        """conditions on the INPUTS, from the reference alone: enough NaN, enough LD, both signs, both orientations"""
        r2 = self.band[0]
        nan = int(np.isnan(r2).sum())
        strong = int((r2[~np.isnan(r2)] >= 0.2).sum())
        cov = self.stats[:, 5] * self.stats[:, 0] - self.stats[:, 1] * self.stats[:, 3]
        neg = float((cov < 0).mean())
        alt_major = int(((self.raw == 2).sum(1) > (self.raw == 0).sum(1)).sum())
        print("fixture (%d, %d): %d pairs, %d NaN, %d with r^2 >= 0.2, %.1f %% negative covariance, %d ALT-major rows"
              % (self.m, self.n, len(r2), nan, strong, 100 * neg, alt_major))
        assert (self.stats[:, 0] == self.n).all()
        if self.n >= 90:
            assert nan >= 1000 and strong >= 500
            assert 0.25 <= neg <= 0.75
            assert 0.25 * self.m <= alt_major <= 0.75 * self.m

    def hits(self, mode, thr, r0, rc, c0, cc):
        """the reference's filtered list for rows [r0, +rc) x columns [c0, +cc), sorted by (first, second)"""
        v = self.band[mode]
        with np.errstate(invalid="ignore"):
            sel = (self.second >= r0) & (self.second < r0 + rc) & (self.first >= c0) & (self.first < c0 + cc) & (np.abs(v) >= thr)
        f, s, v = self.first[sel], self.second[sel], v[sel]
        order = np.lexsort((s, f))
        return f[order], s[order], v[order]


_REFS = {}


def reference(m, n):
    if (m, n) not in _REFS:
        _REFS[(m, n)] = Reference(m, n)
    return _REFS[(m, n)]


def tiles_expected(options, row_first, row_ct):
    """the planner's rule: windows start at 0 in the all-pairs plan, so the reach is the block index of the last requested row"""
    return (row_first + row_ct - 1) // 32 >= options.get("wide_min_reach", K_WIDE_MIN_REACH)


def planned(m, row_first, row_ct, col_first=0, col_end=None):
    """What the all-pairs plan of a request holds, from its definition (plan_mfma_generic with lo = 0): one 32 x 32 block product (a, b) for
    every row-block a with a requested second variant that has a partner (any but variant 0), and every row-block b <= a that overlaps the
    requested columns.  Returns (products, 8 x 8 tiles that hold at least one of them)."""
    col_end = m if col_end is None else col_end
    products, tiles = 0, set()
    for a in range(row_first // 32, (row_first + row_ct - 1) // 32 + 1):
        if min(row_first + row_ct, 32 * a + 32, m) - 1 < 1:
            continue
        for b in range(a + 1):
            if (32 * b < col_end) and (32 * b + 32 > col_first):
                products += 1
                tiles.add((a // 8, b // 8))
    return products, len(tiles)


class Engine:
    def __init__(self, pkg, ref, options):
        self.pkg, self.ref, self.options = pkg, ref, options
        self.eng = pkg.LdPruneEngine(ref.n, 2, 1, False, 0.5, device=0)
        for name, value in options.items():
            self.eng.set_option(name, value)
        self.eng.set_variants_matrix(ref.m)
        self.eng.load_genotypes_host(0, ref.packed, pkg.LDP_GENO_REF)
        self.compared = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.close()
        TOTALS["compared"] += self.compared

    def ran(self, row_first, row_ct, what, col_first=0, col_end=None):
        """the counters of the call just made: complete route, tiles exactly where the rule says, the planned products and tiles those of
        the requested rows x columns and no others (a product planned outside the columns would be clipped pair by pair in the epilogue:
        right values, wasted work)"""
        c = self.eng.counters()
        products, tiles = planned(self.ref.m, row_first, row_ct, col_first, col_end)
        assert c["mfma_block_products"] == products, (what, self.options, row_first, row_ct, col_first, col_end, c["mfma_block_products"], products)
        if tiles_expected(self.options, row_first, row_ct):
            assert c["wide_tiles"] == tiles, (what, self.options, row_first, row_ct, col_first, col_end, c["wide_tiles"], tiles)
        where = (what, self.options, row_first, row_ct, {k: c[k] for k in ("route_complete_launches", "route_general_launches", "route_sparse_launches",
                                                                            "wide_tiles", "mfma_block_products")})
        assert (c["route_complete_launches"], c["route_general_launches"], c["route_sparse_launches"]) == (1, 0, 0), where
        assert (c["wide_tiles"] > 0) == tiles_expected(self.options, row_first, row_ct), where
        assert c["mfma_block_products"] > 0, where
        TOTALS["calls"] += 1
        return c

    def same(self, got, want, what, r0, c0):
        """bit patterns of two dense arrays; a failure names the first pairs"""
        gb, wb = T.bits_of(got), T.bits_of(want)
        assert gb.shape == wb.shape, (what, gb.shape, wb.shape)
        bad = np.argwhere(gb != wb)
        if len(bad):
            lines = ["%s %s: %d of %d elements differ" % (what, self.options, len(bad), gb.size)]
            for q, p in bad[:10]:
                i, j = c0 + int(p), r0 + int(q)
                st = tuple(int(x) for x in self.ref.full_stats[j, i].tolist()) if i < j else None
                lines.append("  pair (i=%d, j=%d): got %r (0x%x) want %r (0x%x); nm,sum1,ssq1,sum2,ssq2,dot = %s"
                             % (i, j, got[q, p], int(gb[q, p]), want[q, p], int(wb[q, p]), st))
            lines.append("  counters: %s" % {k: v for k, v in self.eng.counters().items() if k.startswith("route_") or k in ("wide_tiles", "mfma_block_products")})
            pytest.fail("\n".join(lines))
        self.compared += int(np.tril(np.ones(gb.shape, dtype=bool), (r0 - c0) - 1).sum())   # the pairs i < j inside the block

    def rows(self, mode, r0, rc, as_float):
        got = self.eng.r2_unphased_rows(r0, rc, as_float=as_float)
        self.ran(r0, rc, "rows")
        full = (self.ref.full32 if as_float else self.ref.full)[mode]
        self.same(got, full[r0:r0 + rc, :r0 + rc], "rows(%d, %d, float=%s, signed=%d)" % (r0, rc, as_float, mode), r0, 0)
        return got

    def block(self, mode, r0, rc, c0, cc, as_float):
        got = self.eng.r2_unphased_block(r0, rc, c0, cc, as_float=as_float)
        self.ran(r0, rc, "block", c0, c0 + cc)
        full = (self.ref.full32 if as_float else self.ref.full)[mode]
        self.same(got, full[r0:r0 + rc, c0:c0 + cc], "block(%d, %d, %d, %d, float=%s, signed=%d)" % (r0, rc, c0, cc, as_float, mode), r0, c0)

    def tuples(self, r0, rc, c0, cc):
        got = self.eng.pair_stats_block(r0, rc, c0, cc)
        self.ran(r0, rc, "pair_stats_block", c0, c0 + cc)
        want = self.ref.full_stats[r0:r0 + rc, c0:c0 + cc]
        for name in T.PAIR_FIELDS:
            bad = np.argwhere(got[name].astype(np.int64) != want[name])
            assert not len(bad), ("pair_stats_block(%d, %d, %d, %d) %s" % (r0, rc, c0, cc, self.options), name,
                                  [(c0 + int(p), r0 + int(q), got[q, p].tolist(), want[q, p].tolist()) for q, p in bad[:10]])
        self.compared += int(np.tril(np.ones(got.shape, dtype=bool), (r0 - c0) - 1).sum())

    def hits(self, mode, thr, r0, rc, c0=None, cc=None, capacity=1 << 18):
        if c0 is None:
            got, found = self.eng.r2_unphased_hits(thr, r0, rc, capacity=capacity)
            c0, cc, what = 0, self.ref.m, "hits(%g, %d, %d, signed=%d)" % (thr, r0, rc, mode)
        else:
            got, found = self.eng.r2_unphased_block_hits(thr, r0, rc, c0, cc, capacity=capacity)
            what = "block_hits(%g, %d, %d, %d, %d, signed=%d)" % (thr, r0, rc, c0, cc, mode)
        self.ran(r0, rc, what, c0, c0 + cc)
        f, s, v = self.ref.hits(mode, thr, r0, rc, c0, cc)
        assert found == len(f), (what, self.options, "found", found, "reference", len(f))
        if capacity < len(f):                         # overflow: `capacity` entries, all of them members of the reference's list
            assert len(got) == capacity
            members = {(int(a), int(b)): int(x) for a, b, x in zip(f, s, T.bits_of(v))}
            for h in got:
                assert members.get((int(h["first"]), int(h["second"]))) == int(T.bits_of(np.float64(h["r2"]))[0]), (what, self.options, h)
            return
        assert len(got) == len(f), (what, self.options, len(got), len(f))
        gf, gs = got["first"].astype(np.int64), got["second"].astype(np.int64)
        assert np.array_equal(gf, f) and np.array_equal(gs, s), (what, self.options, "pair sets differ",
                                                                 sorted(set(zip(gf.tolist(), gs.tolist())) ^ set(zip(f.tolist(), s.tolist())))[:10])
        bad = np.flatnonzero(T.bits_of(got["r2"]) != T.bits_of(v))
        assert not len(bad), (what, self.options, [(int(f[k]), int(s[k]), got["r2"][k], v[k]) for k in bad[:10]])
        self.compared += len(f)


def clip(shape, m):
    """a (row_first, row_ct[, col_first, col_ct]) request of the m = 600 list, cut to a smaller matrix"""
    r0, rc = min(shape[0], m - 1), shape[1]
    rc = min(rc, m - r0)
    if len(shape) == 2:
        return (r0, rc)
    c0 = min(shape[2], m - 1)
    return (r0, rc, c0, min(shape[3], m - c0))


CHUNKS = [(0, 300), (257, 100), (599, 1), (384, 216)]
BLOCKS = [(0, 600, 0, 600), (300, 300, 0, 300), (257, 100, 31, 200), (512, 88, 256, 256), (400, 150, 390, 100), (599, 1, 0, 599), (33, 1, 0, 33)]
SAMPLE_COUNTS = [3, 90, 512, 513, 1100]


def finish(t0, label, compared):
    dt = time.time() - t0
    TOTALS["seconds"] += dt
    print("pairs compared: %d  (%s; %.2f s)" % (compared, label, dt))


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


# ---------------------------------------------------------------- the windowed plan
WINDOWS = [(1 << 30, 0x7fffffff), (1 << 30, 40), (900, 3)]


def windowed_positions(m):
    rng = np.random.default_rng(3)
    chr_idx = np.repeat(np.arange(3), [250, 1, m - 251]).astype(np.uint32)
    bps = np.zeros(m, dtype=np.uint32)
    for c in range(3):
        sel = np.where(chr_idx == c)[0]
        bps[sel] = np.sort(rng.integers(1, 40000, size=len(sel)))
    return chr_idx, bps


_BAND_REFS = {}


def band_reference(ref, lo):
    key = (ref.n, lo.tobytes())
    if key not in _BAND_REFS:
        _BAND_REFS[key] = T.band_r2(T.band_pair_stats(ref.raw, lo))
        _BAND_REFS[key].setflags(write=False)
    return _BAND_REFS[key]


@pytest.mark.parametrize("bp_radius,var_radius", WINDOWS)
@pytest.mark.parametrize("n", [90, 1100])
def test_windowed_plan(gpu_pkg, n, bp_radius, var_radius):
    """set_variants_vcor over chromosome runs [250, 1, 349]: launches without tiles, pair_mfma_kernel<4, false, diag> and its general-form
    sibling -- whole-chromosome windows (reach up to 10 blocks, several wave items per block pair), 40 variants, and a narrow bp window.
    band()'s lo against UpdateVcorWindow's rule; band rows whole and in chunks, doubles and floats; hits with global indices."""
    t0 = time.time()
    pkg = gpu_pkg
    m = 600
    ref = reference(m, n)
    chr_idx, bps = windowed_positions(m)
    eng = pkg.LdPruneEngine(n, 2, 1, False, 0.5, device=0)
    eng.set_variants_vcor(chr_idx, bps, bp_radius, var_radius)
    eng.load_genotypes_host(0, ref.packed, pkg.LDP_GENO_REF)
    lo, cand = eng.band()
    for j in range(m):
        i = j
        while i > 0 and chr_idx[i - 1] == chr_idx[j] and int(bps[j]) - int(bps[i - 1]) <= bp_radius and j - (i - 1) <= var_radius:
            i -= 1
        assert lo[j] == i, (j, lo[j], i)
    lo = lo.astype(np.int64)
    first, second = T.band_pairs(lo)
    assert len(first) == cand > 500
    want = band_reference(ref, lo)
    off = np.concatenate([[0], np.cumsum(np.arange(m) - lo)])
    compared = 0

    def complete_route(what):
        c = eng.counters()
        assert (c["route_complete_launches"], c["route_general_launches"], c["route_sparse_launches"], c["wide_tiles"]) == (1, 0, 0, 0), (what, c)
        assert c["mfma_block_products"] > 0

    for r0, cnt in ((0, m), (37, 101), (m - 5, 5)):
        w = want[off[r0]:off[r0 + cnt]]
        for as_float in (False, True):
            got = eng.r2_unphased_band_rows(r0, cnt, as_float=as_float)
            complete_route("band rows")
            wv = T.r2_to_float32(w) if as_float else w
            bad = np.flatnonzero(T.bits_of(got) != T.bits_of(wv))
            assert got.shape == wv.shape and not len(bad), ((r0, cnt, as_float), [(int(first[off[r0] + k]), int(second[off[r0] + k]), got[k], wv[k]) for k in bad[:10]])
            compared += len(w)
    for thr, r0, cnt in ((0.2, 0, m), (0.0, 0, m), (1e-9, 37, 101), (0.2, m - 5, 5)):
        hits, found = eng.r2_unphased_hits(thr, r0, cnt, capacity=1 << 18)
        complete_route("band hits")
        with np.errstate(invalid="ignore"):
            sel = (second >= r0) & (second < r0 + cnt) & (np.abs(want) >= thr)
        f, s, v = first[sel], second[sel], want[sel]
        order = np.lexsort((s, f))
        assert found == len(f) == len(hits), (thr, r0, cnt, found, len(f), len(hits))
        assert np.array_equal(hits["first"].astype(np.int64), f[order]) and np.array_equal(hits["second"].astype(np.int64), s[order])
        assert np.array_equal(T.bits_of(hits["r2"]), T.bits_of(v[order]))
        compared += len(f)
    eng.close()
    TOTALS["compared"] += compared
    finish(t0, "windowed plan n = %d, window (%d, %d): %d candidate pairs" % (n, bp_radius, var_radius, cand), compared)


def test_zz_totals():
    print("pairs compared in this file: %d over %d counted calls, %.1f s in its tests" % (TOTALS["compared"], TOTALS["calls"], TOTALS["seconds"]))
    assert TOTALS["compared"] > 0 and TOTALS["calls"] > 0
