"""The wave -> rectangle map of the DIAGONAL tiles of pair_mfma_wide_kernel (csrc/ldp_device.h: kWdDiagMap).

A diagonal tile holds the 36 block products on and below the diagonal.  Its 2 x 3 body gives every wave one rectangle of J blocks a0, a0 + 1 x V blocks
b0 .. b0 + 2 and the products of some of its columns to OWN; the near rectangles (every product on and next to the block diagonal) sit on waves 0-3, one
per SIMD, the rest on waves 4-7, so the tail of a tile behind its checkpoints runs on four waves.  An ownership error shows as a pair decided twice
(pred_true counts it twice), never (a missing bit), or by a wave that has stopped (a missing bit on a pair in LD far from the diagonal).

CPU: the table the library exports (ldp_debug_wide_diag_map -- the one the kernel's constants are made from) is a partition.
GPU: every candidate pair's decision, at the smallest shapes that reach this code with two checkpoints and a tail behind them."""
import numpy as np
import pytest

import ldtools as T

BLOCK, TILE = 32, 8


# ---------------------------------------------------------------- CPU: the exported table
def test_the_exported_map_partitions_the_triangle(pkg):
    words = pkg.LdPruneEngine.debug_wide_diag_map()
    assert words.shape == (8, 5)
    seen = {}
    for w, (a0, b0, cols, lo, hi) in enumerate(words.tolist()):
        assert a0 + 1 < TILE and b0 + 3 <= TILE and 0 < cols < 8, (w, a0, b0, cols)   # the rectangle lies inside the tile (no V block 8)
        owned = lo | (hi << 32)
        want = 0
        for j in (a0, a0 + 1):
            for b in range(3):
                if (cols >> b) & 1 and (b0 + b <= j):
                    want |= 1 << (8 * j + b0 + b)
        assert owned == want, (w, hex(owned), hex(want))        # every owned product lies inside the wave's 2 x 3 rectangle, in an owned column
        for bit in range(64):
            if (owned >> bit) & 1:
                assert bit not in seen, "product (%d, %d) owned by waves %d and %d" % (bit >> 3, bit & 7, seen[bit], w)
                seen[bit] = w
    triangle = {8 * j + v for j in range(TILE) for v in range(j + 1)}
    assert set(seen) == triangle and len(seen) == 36
    # the products that outlive the checkpoints -- on and next to the block diagonal -- are on waves 0-3: one wave per SIMD (waves w, w + 4 share one)
    for j in range(TILE):
        for v in range(max(j - 1, 0), j + 1):
            assert seen[8 * j + v] < 4, (j, v, seen[8 * j + v])
    # ... and waves 4-7 hold nothing closer than two blocks
    assert all((bit >> 3) - (bit & 7) >= 2 for bit, w in seen.items() if w >= 4)
    assert sum(1 for w in seen.values() if w < 4) == 18


def test_the_map_hook_refuses_a_short_buffer(pkg):
    import ctypes
    buf = np.zeros(40, dtype=np.uint32)
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    assert pkg.lib().ldp_debug_wide_diag_map(p, 39) == pkg.LDP_ERR_INVALID
    assert pkg.lib().ldp_debug_wide_diag_map(None, 40) == pkg.LDP_ERR_INVALID
    assert pkg.lib().ldp_debug_wide_diag_map(p, 40) == pkg.LDP_OK


# ---------------------------------------------------------------- GPU: decisions on the production kernel
# Two subcontigs of 768 and 1,100 variants: three and five J tiles of 256, the last one ragged (76 rows: two whole blocks and 12 rows of a third).
# A count window of 400 variants reaches 13 row-blocks >= kWdMinReach (12), so both take the tile plan by themselves.
SUBCONTIGS = (768, 1100)
M = sum(SUBCONTIGS)
WINDOW = 400
SAMPLES = (4608, 9000)     # nine whole 512-sample stages; 18 stages with a ragged last one
CHAINS = {}                # genotype set -> [(first row, length)] (for the assertions on what a set exercises)


def _fresh(rng, rows, n, maf_lo=0.1):
    maf = rng.uniform(maf_lo, 0.5, size=(rows, 1))
    flip = rng.random((rows, 1)) < 0.5       # ALT is the major allele in half of the rows
    maf = np.where(flip, 1.0 - maf, maf)
    return ((rng.random((rows, n)) < maf).astype(np.uint8) + (rng.random((rows, n)) < maf).astype(np.uint8))


def _chain(rng, raw, first, length, redraw):
    """rows first + 1 .. first + length - 1 copy their predecessor, `redraw` of the samples drawn anew: r^2 falls by about (1 - redraw)^2 per row"""
    n = raw.shape[1]
    for v in range(first + 1, first + length):
        keep = rng.random(n) >= redraw
        raw[v] = np.where(keep, raw[v - 1], _fresh(rng, 1, n)[0])


def genotypes(kind, n):
    """complete REF-based codes (M, n), built in numpy"""
    rng = np.random.default_rng(1000 * n + {"none": 1, "short": 2, "long": 3}[kind])
    raw = _fresh(rng, M, n)
    chains = []
    if kind == "short":
        # chains of five rows across every 32-row block boundary of both subcontigs -- the tile boundaries (multiples of 256) among them --, and one
        # ending on / one starting at a boundary
        for s0, slen in zip((0, SUBCONTIGS[0]), SUBCONTIGS):
            for b in range(BLOCK, slen - 3, BLOCK):
                chains.append((s0 + b - 2 - (b // BLOCK) % 2, 5))
            chains.append((s0 + 3 * BLOCK + 8, 5))
        for first, length in chains:
            _chain(rng, raw, first, length, 0.06)
    elif kind == "long":
        # chains of about 80 rows, r^2 still above 0.2 end to end: pairs in LD two and three row-blocks apart, in products the REST waves own.
        #   subcontig 2, rows 266 .. 345: blocks 0-2 of its second diagonal tile -> product (2, 0)
        #   subcontig 1, rows 150 .. 233: blocks 4-7 of its first diagonal tile -> products (6, 4) and (7, 4), (7, 5), beside near products
        #   subcontig 2, rows 720 .. 799: across the boundary of J tiles 2 and 3 -> the distance-1 tile's corner and (1, 0) / (2, 0) of tile 3
        chains = [(SUBCONTIGS[0] + 266, 80), (150, 84), (SUBCONTIGS[0] + 720, 80)]
        for first, length in chains:
            _chain(rng, raw, first, length, 0.005)
    CHAINS[kind] = chains
    assert not (raw == 3).any()
    return raw


class Rows:
    """one genotype set at one sample count, and everything the engines over it are compared with -- computed once"""

    def __init__(self, pkg, kind, n):
        self.kind, self.n = kind, n
        self.raw = genotypes(kind, n)
        self.packed = T.pack_2bit(self.raw)
        self.chr_idx = np.repeat(np.arange(2, dtype=np.uint32), SUBCONTIGS)
        eng = pkg.LdPruneEngine(n, WINDOW, 1, False, 0.2, order=2, device=0)
        eng.set_option("wide_min_reach", 12)
        eng.set_variants(self.chr_idx, None)
        self.lo, self.cand = eng.band()
        self.plan = eng.debug_wide_plan()
        eng.close()
        self.stats = T.band_pair_stats(self.raw, self.lo)
        assert len(self.stats) == self.cand
        self.inv, self.mf, _ = T.oracle_prepare(self.raw)
        self.first, self.second = T.band_pairs(self.lo)
        self._dec, self._removed = {}, {}

    def decisions(self, r2):
        if r2 not in self._dec:
            self._dec[r2] = T.band_decisions(self.stats, r2)
        return self._dec[r2]

    def removed(self, r2, order):
        if (r2, order) not in self._removed:
            self._removed[(r2, order)] = T.oracle_indep_pairwise(self.inv, self.n, self.chr_idx, np.arange(M, dtype=np.uint32), self.mf, WINDOW, 1, False, r2, order)[0]
        return self._removed[(r2, order)]


_ROWS = {}


def rows_of(pkg, kind, n):
    if (kind, n) not in _ROWS:
        _ROWS[(kind, n)] = Rows(pkg, kind, n)
    return _ROWS[(kind, n)]


def run(pkg, rows, r2, order, diag_kernel):
    eng = pkg.LdPruneEngine(rows.n, WINDOW, 1, False, r2, order=order, device=0)
    eng.set_option("wide_min_reach", 12)
    eng.set_option("wide_diag_kernel", diag_kernel)
    eng.set_variants(rows.chr_idx, None)
    eng.load_genotypes_host(0, rows.packed, pkg.LDP_GENO_REF)
    removed = eng.run()
    pred, outside = eng.last_pred(with_outside=True)
    c = eng.counters()
    eng.close()
    return removed, pred, outside, c


@pytest.mark.gpu
@pytest.mark.parametrize("order", [2, 1])
@pytest.mark.parametrize("r2", [0.2, 0.5])
@pytest.mark.parametrize("n", SAMPLES)
@pytest.mark.parametrize("kind", ["none", "short", "long"])
def test_every_decision_of_the_diagonal_tiles(gpu_pkg, kind, n, r2, order):
    """kind "none": no LD at all, every wave retires at the first checkpoint.  "short": copy chains of five rows across every 32-row block boundary and every
    256-row tile boundary: the near waves' products stay, the rest waves retire.  "long": chains of about 80 rows: pairs in LD two and three blocks
    apart, in products the REST waves own, which must then live on past the checkpoints (the bench line's generator never does this)."""
    pkg = gpu_pkg
    rows = rows_of(pkg, kind, n)
    want = rows.decisions(r2)
    # the plan: 3 + 5 diagonal tiles, each with the whole (ragged) triangle live
    diag = rows.plan[rows.plan[:, 0] == rows.plan[:, 1]]
    assert len(diag) == 8 and len(rows.plan) > len(diag)
    # what the set exercises, from the reference alone
    s0 =np.where(rows.second >= SUBCONTIGS[0], SUBCONTIGS[0], 0)
    block_dist = (rows.second - s0) // BLOCK - (rows.first - s0) // BLOCK
    if kind == "none":
        assert not want.any()
    elif kind == "short":
        assert want.any() and (block_dist[want] <= 1).all() and (block_dist[want] == 1).any()
        tile_crossers = want & ((rows.second - s0) // (BLOCK * TILE) != (rows.first - s0) // (BLOCK * TILE))
        assert tile_crossers.any()
    else:
        assert (want & (block_dist >= 2)).any()       # pairs in LD in the rest waves' products
        if r2 <= 0.2:
            assert (want & (block_dist >= 3)).any()
    results = {}
    for dk in (1, 0):
        removed, pred, outside, c = run(pkg, rows, r2, order, dk)
        print("pairs compared: %d (%s, n %d, r2 %g, order %d, wide_diag_kernel %d; %d true; wide tiles %d, skipped product stages %d, extra %d)"
              % (len(pred), kind, n, r2, order, dk, int(pred.sum()), c["wide_tiles"], c["mfma_skipped_product_stages"], c["mfma_extra_product_stages"]))
        assert c["candidate_pairs"] == rows.cand == len(pred)
        nd, msg = T.compare_decisions(pred, want, rows.lo, rows.stats, r2, counters=c)
        assert nd == 0, "wide_diag_kernel %d\n%s" % (dk, msg)
        assert int(pred.sum()) == c["pred_true"], (dk, int(pred.sum()), c["pred_true"])     # every pair owned and counted once
        assert outside == 0
        assert np.array_equal(removed, rows.removed(r2, order)), (dk, int(removed.sum()), int(rows.removed(r2, order).sum()))
        assert c["route_complete_launches"] > 0 and c["route_sparse_launches"] == 0 and c["route_general_launches"] == 0
        assert c["wide_tiles"] > 0
        assert c["mfma_skipped_product_stages"] > 0      # the checkpoints retired products: there was a tail
        results[dk] = (pred, removed)
    assert np.array_equal(results[1][0], results[0][0]) and np.array_equal(results[1][1], results[0][1])
