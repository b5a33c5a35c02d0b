"""Shared by the tests of the r^2 outputs (test_r2_complete.py, test_r2_missing.py, test_pair_reference.py): the fixtures' rows, the reference of
everything an engine over them must return (ldtools.band_pair_stats / band_r2: float64 matrix products and ComputeR2's operations in numpy, which
tests/test_pair_reference.py checks against the oracle on the CPU), the planner's rules restated from their definition, and an engine wrapper
whose every call is compared pair by pair -- no sampling, no tolerance, bit patterns only -- and proves from the counters of the call itself
(include/ldprune_hip.h) which kernel ran.  Nothing here is derived from the code under test."""
import time

import numpy as np
import pytest

import ldtools as T

K_WIDE_MIN_REACH = 12      # row-blocks of 32 (kWdMinReach): the all-pairs plan takes tiles when the last requested row's block index reaches it

# the expected (route_complete_launches, route_general_launches, route_sparse_launches) of a call
ROUTE_COMPLETE = (1, 0, 0)   # no missing call in the resident rows: pair_mfma_kernel<4, false, *> and, where planned, the 8 x 8 tiles
ROUTE_GENERAL = (0, 1, 0)    # one missing call anywhere: pair_mfma_general_kernel<true, false>, the tile plan standing by
ROUTE_POPCOUNT = (0, 0, 0)   # option pair_mfma 0: the popcount kernels; report_r2_plan leaves all five counters zero

ROUTE_COUNTERS = ("route_complete_launches", "route_general_launches", "route_sparse_launches", "wide_tiles", "mfma_block_products")


def new_totals():
    """one per test file: pairs compared, counted calls, seconds and parametrised cases that ran to their end"""
    return {"compared": 0, "calls": 0, "seconds": 0.0, "cases": 0}


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


MISSING_RATES = (0.0, 0.001, 0.02, 0.2, 0.6)
MISSING_RATE_PROBS = (0.35, 0.2, 0.2, 0.15, 0.1)


def missing_places(m):
    """the rows missing_rows(m, n) places missing calls in deliberately, those that fall inside m rows: all-missing rows, complementary pairs,
    pairs whose first row varies only where the second is missing, rows with missing calls at the sample edges, rows with one carrier"""
    inside = lambda pairs: [p for p in pairs if max(p) < m]
    return {"all_missing": sorted({v for v in (17, 300, m - 3) if 0 <= v < m}),
            "complementary": inside([(50, 290), (258, 259), (31, 32)]),     # across tiles, inside a row-block, across a row-block boundary
            "shared_variance": inside([(70, 330), (513, 515)]),
            "edges": sorted({v for v in (100, 257, m - 1) if 0 <= v < m}),
            "singletons": [v for v in (110, 521) if v < m]}


def missing_rows(m, n, seed=11):
    """complete_rows(m, n) -- its LD families, both orientations, its monomorphic rows -- with missing calls, all from one seeded generator:
    * every row misses 0, 0.1 %, 2 %, 20 % or 60 % of its calls (probabilities 0.35, 0.2, 0.2, 0.15, 0.1): complete, nearly complete and badly
      called rows meet in every block product, and the major allele of many rows is decided by the calls they have;
    * row 26 keeps its exact REF = ALT tie, now among an even number of calls in front of one or two missing ones;
    * rows 17, 300 and m - 3 have no call at all;
    * (50, 290), (258, 259), (31, 32): the first row is missing on samples [0, n/2), the second on [n/2, n) -- both rows have calls, the pair
      has nm == 0;
    * (70, 330), (513, 515): the first row is hom-REF except hom-ALT on samples [0, 5), where the second is missing -- the first row has a
      variance of its own and none over the shared samples: NaN through variance_prod == 0.0, not through nm == 0;
    * rows 100, 257 and m - 1 miss the call of sample n - 1 (the last code of the row; its byte is shared with padding when n % 4 != 0) and of
      samples 511 (n >= 512) and 512 (n > 512), the two sides of the first 512-sample stage boundary;
    * rows 110 and 521 are singletons, complete and hom-REF but for one het call at sample n - 1 (110) and one hom-ALT call at sample 0 (521):
      a variance of their own, none with any partner that misses that one sample -- some 50 pairs each at every n, where the draws alone leave
      fewer and fewer such pairs as n grows.
    Rows outside a smaller m are skipped."""
    raw = complete_rows(m, n).copy()
    complete = raw.copy()
    rng = np.random.default_rng(seed + 1000 * m + n)
    rates = rng.choice(MISSING_RATES, size=m, p=MISSING_RATE_PROBS)
    raw[rng.random((m, n)) < rates[:, None]] = 3
    places = missing_places(m)
    calls = (n - 1) & ~1                               # row 26: the largest even number of calls that leaves one missing
    raw[26] = 3
    raw[26, :calls] = 0
    raw[26, : calls // 2] = 2
    for v in places["all_missing"]:
        raw[v] = 3
    for a, b in places["complementary"]:
        raw[a], raw[b] = complete[a], complete[b]
        raw[a, : n // 2] = 3
        raw[b, n // 2:] = 3
    for a, b in places["shared_variance"]:
        raw[a] = 0
        raw[a, :5] = 2
        raw[b, :5] = 3
    for v in places["singletons"]:
        raw[v] = 0
        raw[v, n - 1 if v == 110 else 0] = 1 if v == 110 else 2
    for v in places["edges"]:
        raw[v, n - 1] = 3
        if n > 512:
            raw[v, 512] = 3
        if n >= 512:
            raw[v, 511] = 3
    return raw


def alt_major(raw):
    """the rows whose major allele is ALT, by the allele counts of their calls (ldtools.band_pair_stats' rule, restated: ref_freq < 0.5)"""
    ref_ct = 2 * (raw == 0).sum(1).astype(np.int64) + (raw == 1).sum(1)
    alt_ct = 2 * (raw == 2).sum(1).astype(np.int64) + (raw == 1).sum(1)
    tot = ref_ct + alt_ct
    return np.where(tot > 0, ref_ct.astype(np.float64) * (1.0 / np.maximum(tot, 1).astype(np.float64)), 0.5) < 0.5


class Reference:
    """one fixture and everything the engines over it must return: computed once per (m, n), never changed"""

    def __init__(self, m, n, raw=None):
        self.m, self.n = m, n
        self.raw = self.rows_of(m, n) if raw is None else np.array(raw, dtype=np.uint8)
        assert self.raw.shape == (m, n)
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

    rows_of = staticmethod(complete_rows)

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

    def pair(self, i, j):
        """band index of the pair i < j"""
        return j * (j - 1) // 2 + i

    def hits(self, mode, thr, r0, rc, c0, cc):
        """the reference's filtered list for rows [r0, +rc) x columns [c0, +cc), sorted by (first, second)"""
        v = self.band[mode]
        with np.errstate(invalid="ignore"):
            sel = (self.second >= r0) & (self.second < r0 + rc) & (self.first >= c0) & (self.first < c0 + cc) & (np.abs(v) >= thr)
        f, s, v = self.first[sel], self.second[sel], v[sel]
        order = np.lexsort((s, f))
        return f[order], s[order], v[order]


class MissingReference(Reference):
    """missing_rows(m, n)"""
    rows_of = staticmethod(missing_rows)

    def input_conditions(self):
        """Conditions on the INPUTS, from the reference alone.  The placed rows are checked at every shape.  The shares (negative covariance,
        complete rows, pairs with nm < n, every block product) hold from n = 90 on at every m; the counts are those of m = 600, whose 179,700
        pairs they were set for (three all-missing rows alone give 1,794 pairs with nm == 0; m = 200 has two such rows and 79,600 pairs less)."""
        m, n, raw, st = self.m, self.n, self.raw, self.stats
        r2 = self.band[0]
        nm = st[:, 0]
        calls = (raw != 3).sum(1)
        own_var = ~np.isnan(self.diag)
        places = missing_places(m)
        for v in places["all_missing"]:
            assert calls[v] == 0 and np.isnan(self.diag[v])
            assert (nm[(self.first == v) | (self.second == v)] == 0).all()
        for a, b in places["complementary"]:
            assert calls[a] > 0 and calls[b] > 0 and calls[a] + calls[b] == n
            assert nm[self.pair(a, b)] == 0 and np.isnan(r2[self.pair(a, b)])
        for a, b in places["shared_variance"]:
            assert np.isnan(r2[self.pair(a, b)])
            if n > 5:
                k = self.pair(a, b)
                assert own_var[a] and nm[k] == calls[b] > 0 and st[k, 2] * nm[k] - st[k, 1] * st[k, 1] == 0
        for v in places["edges"]:
            assert raw[v, n - 1] == 3 and (n < 512 or raw[v, 511] == 3) and (n <= 512 or raw[v, 512] == 3)
        for v in places["singletons"]:
            assert calls[v] == n and own_var[v] and (raw[v] != 0).sum() == 1
            k = (self.first == v) | (self.second == v)
            assert n < 90 or (np.isnan(r2[k]) & (nm[k] > 0)).sum() >= 20
        assert 0 < calls[26] < n and calls[26] % 2 == 0 and (raw[26] == 0).sum() == (raw[26] == 2).sum() == calls[26] // 2

        nm0 = int((nm == 0).sum())
        nan_own = int((np.isnan(r2) & (nm > 0) & own_var[self.first] & own_var[self.second]).sum())
        strong = int((r2[~np.isnan(r2)] >= 0.2).sum())
        cov = st[:, 5] * nm - st[:, 1] * st[:, 3]
        neg = float((cov < 0).mean())
        complete = int((calls == n).sum())
        partial = nm < n
        blocks = np.zeros(((m + 31) // 32, (m + 31) // 32), dtype=bool)
        blocks[self.second[partial] // 32, self.first[partial] // 32] = True
        wanted = np.zeros_like(blocks)
        wanted[self.second // 32, self.first // 32] = True          # (every block product of the lower triangle that holds a pair)
        self.counts = {"nm0": nm0, "nan_own_variance": nan_own, "strong": strong, "negative": neg, "complete_rows": complete, "partial": int(partial.sum())}
        print("fixture with missing calls (%d, %d): %d pairs, %d with nm == 0, %d NaN with nm > 0 and a variance of both rows, %d with r^2 >= 0.2, "
              "%.1f %% negative covariance, %d complete rows, %d pairs with nm < n, %d of %d block products hold one"
              % (m, n, len(r2), nm0, nan_own, strong, 100 * neg, complete, int(partial.sum()), int((blocks & wanted).sum()), int(wanted.sum())))
        if n >= 90:
            assert 0.25 <= neg <= 0.75
            assert complete >= 0.25 * m
            assert 2 * int(partial.sum()) >= len(r2)
            assert (blocks & wanted).sum() == wanted.sum()
            if m == 600:
                assert nm0 >= 1500 and nan_own >= 20 and strong >= 500


_REFS = {}


def reference(m, n):
    if (m, n) not in _REFS:
        _REFS[(m, n)] = Reference(m, n)
    return _REFS[(m, n)]


def reference_missing(m, n):
    if ("missing", m, n) not in _REFS:
        _REFS[("missing", m, n)] = MissingReference(m, n)
    return _REFS[("missing", m, n)]


class OneMissingReference(Reference):
    """complete_rows(m, n) with exactly one missing call"""

    def input_conditions(self):
        assert int((self.raw == 3).sum()) == 1
        assert int((self.stats[:, 0] == self.n - 1).sum()) == self.m - 1 and int((self.stats[:, 0] == self.n).sum()) == len(self.stats) - (self.m - 1)


def reference_one_missing(m, n, row, sample):
    key = ("one", m, n, row, sample)
    if key not in _REFS:
        raw = complete_rows(m, n).copy()
        raw[row, sample] = 3
        _REFS[key] = OneMissingReference(m, n, raw)
    return _REFS[key]


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
    """An engine over a Reference's rows in the all-pairs plan.  route: what every call's counters must say ran (ROUTE_COMPLETE, ROUTE_GENERAL,
    ROUTE_POPCOUNT); totals: the test file's new_totals()."""

    def __init__(self, pkg, ref, options, route, totals):
        self.pkg, self.ref, self.options, self.route, self.totals = pkg, ref, options, route, totals
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
        self.totals["compared"] += self.compared

    def ran(self, row_first, row_ct, what, col_first=0, col_end=None, *, route):
        """the counters of the call just made: the expected route (`route`: complete, general, sparse launches), tiles exactly where the rule
        says -- on a general launch the stand-by plan, which must be attached there all the same --, the planned products and tiles those of
        the requested rows x columns and no others (a product planned outside the columns would be clipped pair by pair in the epilogue:
        right values, wasted work).  The popcount kernels' calls (ROUTE_POPCOUNT) report zeros in all five."""
        c = self.eng.counters()
        if route == ROUTE_POPCOUNT:
            assert all(c[k] == 0 for k in ROUTE_COUNTERS), (what, self.options, row_first, row_ct, {k: c[k] for k in ROUTE_COUNTERS})
            self.totals["calls"] += 1
            return c
        products, tiles = planned(self.ref.m, row_first, row_ct, col_first, col_end)
        assert c["mfma_block_products"] == products, (what, self.options, row_first, row_ct, col_first, col_end, c["mfma_block_products"], products)
        if tiles_expected(self.options, row_first, row_ct):
            assert c["wide_tiles"] == tiles, (what, self.options, row_first, row_ct, col_first, col_end, c["wide_tiles"], tiles)
        where = (what, self.options, row_first, row_ct, {k: c[k] for k in ROUTE_COUNTERS})
        assert (c["route_complete_launches"], c["route_general_launches"], c["route_sparse_launches"]) == tuple(route), where
        assert (c["wide_tiles"] > 0) == tiles_expected(self.options, row_first, row_ct), where
        assert c["mfma_block_products"] > 0, where
        self.totals["calls"] += 1
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
        self.ran(r0, rc, "rows", route=self.route)
        full = (self.ref.full32 if as_float else self.ref.full)[mode]
        self.same(got, full[r0:r0 + rc, :r0 + rc], "rows(%d, %d, float=%s, signed=%d)" % (r0, rc, as_float, mode), r0, 0)
        return got

    def block(self, mode, r0, rc, c0, cc, as_float):
        got = self.eng.r2_unphased_block(r0, rc, c0, cc, as_float=as_float)
        self.ran(r0, rc, "block", c0, c0 + cc, route=self.route)
        full = (self.ref.full32 if as_float else self.ref.full)[mode]
        self.same(got, full[r0:r0 + rc, c0:c0 + cc], "block(%d, %d, %d, %d, float=%s, signed=%d)" % (r0, rc, c0, cc, as_float, mode), r0, c0)

    def tuples(self, r0, rc, c0, cc):
        got = self.eng.pair_stats_block(r0, rc, c0, cc)
        self.ran(r0, rc, "pair_stats_block", c0, c0 + cc, route=self.route)
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
        self.ran(r0, rc, what, c0, c0 + cc, route=self.route)
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
        assert not len(bad), (what, self.options, [(int(f[k]), int(s[k]), got["r2"][k], v[k], tuple(int(x) for x in self.ref.full_stats[int(s[k]), int(f[k])].tolist()))
                                                   for k in bad[:10]])
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


def finish(totals, t0, label, compared):
    dt = time.time() - t0
    totals["seconds"] += dt
    totals["cases"] += 1
    print("pairs compared: %d  (%s; %.2f s)" % (compared, label, dt))


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
    key = (id(ref), lo.tobytes())
    if key not in _BAND_REFS:
        _BAND_REFS[key] = T.band_r2(T.band_pair_stats(ref.raw, lo))
        _BAND_REFS[key].setflags(write=False)
    return _BAND_REFS[key]


def windowed_plan_case(pkg, ref, bp_radius, var_radius, options, route, totals):
    """set_variants_vcor over chromosome runs [250, 1, 349] of ref's rows: band()'s lo against UpdateVcorWindow's rule; band rows whole and in
    chunks, doubles and floats; hits with global indices; every call's counters `route` + no tile (ROUTE_POPCOUNT: all five zero).
    Returns (candidate pairs, pairs compared)."""
    m, n = ref.m, ref.n
    chr_idx, bps = windowed_positions(m)
    eng = pkg.LdPruneEngine(n, 2, 1, False, 0.5, device=0)
    for name, value in options.items():
        eng.set_option(name, value)
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

    def expected_route(what):
        c = eng.counters()
        if route == ROUTE_POPCOUNT:
            assert all(c[k] == 0 for k in ROUTE_COUNTERS), (what, options, {k: c[k] for k in ROUTE_COUNTERS})
        else:
            assert (c["route_complete_launches"], c["route_general_launches"], c["route_sparse_launches"], c["wide_tiles"]) == tuple(route) + (0,), (what, c)
            assert c["mfma_block_products"] > 0

    for r0, cnt in ((0, m), (37, 101), (m - 5, 5)):
        w = want[off[r0]:off[r0 + cnt]]
        for as_float in (False, True):
            got = eng.r2_unphased_band_rows(r0, cnt, as_float=as_float)
            expected_route("band rows")
            wv = T.r2_to_float32(w) if as_float else w
            bad = np.flatnonzero(T.bits_of(got) != T.bits_of(wv))
            assert got.shape == wv.shape and not len(bad), ((r0, cnt, as_float), [(int(first[off[r0] + k]), int(second[off[r0] + k]), got[k], wv[k]) for k in bad[:10]])
            compared += len(w)
    for thr, r0, cnt in ((0.2, 0, m), (0.0, 0, m), (1e-9, 37, 101), (0.2, m - 5, 5)):
        hits, found = eng.r2_unphased_hits(thr, r0, cnt, capacity=1 << 18)
        expected_route("band hits")
        with np.errstate(invalid="ignore"):
            sel = (second >= r0) & (second < r0 + cnt) & (np.abs(want) >= thr)
        f, s, v = first[sel], second[sel], want[sel]
        order = np.lexsort((s, f))
        assert found == len(f) == len(hits), (thr, r0, cnt, found, len(f), len(hits))
        assert np.array_equal(hits["first"].astype(np.int64), f[order]) and np.array_equal(hits["second"].astype(np.int64), s[order])
        assert np.array_equal(T.bits_of(hits["r2"]), T.bits_of(v[order]))
        compared += len(f)
    eng.close()
    totals["compared"] += compared
    return cand, compared
