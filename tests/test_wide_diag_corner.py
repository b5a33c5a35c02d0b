"""The CORNER product of the wide-band tiles (csrc/ldp_device.h: kWdDiagCornerWave; engine option "wide_diag_corner").

The tile one tile distance from the diagonal, (J tile t, V tile t - 1), holds exactly one block product next to the block diagonal: (J block 0, V block 7),
row-block 8 t against 8 t - 1.  With "wide_diag_corner" 1 (the default) the DIAGONAL tile of J tile t computes it instead -- wave 0's third column reads a
ninth staged row-block, the 32 rows in front of the tile -- and the distance-1 tile drops it.  The plan does not change; the move is a property of the launch.
What can go wrong: a corner pair decided by nobody (the distance-1 tile dropped it, the diagonal tile did not take it), decided twice, decided from the
wrong rows (the ninth slot's address, its checkpoint statistics), a product of the distance-1 tile that stopped with the corner, or a first tile / a ragged
last tile that reads rows it does not have.

CPU: the plan and the exported diagonal map do not depend on the option.
GPU: every candidate pair's decision, at the smallest shapes that reach this code, with the corner moved, kept, and with the 2 x 4 body everywhere."""
import numpy as np
import pytest

import ldtools as T

BLOCK, TILE = 32, 8
TILE_ROWS = BLOCK * TILE

# Three subcontigs of 768, 1,100 and 524 variants: 3, 5 and 3 J tiles of 256, the last ones with 256, 76 and 12 rows.  A count window of 400 variants
# reaches 13 row-blocks >= kWdMinReach (12), so each takes the tile plan by itself.  The first J tile of every subcontig has no neighbour.
SUBCONTIGS = (768, 1100, 524)
STARTS = tuple(int(x) for x in np.concatenate([[0], np.cumsum(SUBCONTIGS)[:-1]]))
M = sum(SUBCONTIGS)
WINDOW = 400
SAMPLES = (4608, 9000)     # nine whole 512-sample stages; 18 stages with a ragged last one
KINDS = ("none", "boundary pairs", "boundary chains", "long")
LONG_BOUNDARY = STARTS[1] + 3 * TILE_ROWS    # the tile boundary the long chain crosses: J tiles 2 | 3 of the second subcontig


def tile_boundaries(every_second=False):
    """global row index of every 256-row tile boundary inside a subcontig (every second one of each subcontig: its odd multiples of 256)"""
    out = []
    for s0, slen in zip(STARTS, SUBCONTIGS):
        for k, b in enumerate(range(TILE_ROWS, slen, TILE_ROWS)):
            if not every_second or (k % 2 == 0):
                out.append(s0 + b)
    return out


# ---------------------------------------------------------------- CPU: the plan and the map do not move
def _plan(pkg, corner):
    eng = pkg.LdPruneEngine(4608, WINDOW, 1, False, 0.2, order=2, device=-1)
    eng.set_option("wide_min_reach", 12)
    if corner is not None:
        eng.set_option("wide_diag_corner", corner)
    eng.set_variants(np.repeat(np.arange(len(SUBCONTIGS), dtype=np.uint32), SUBCONTIGS), None)
    plan = eng.debug_wide_plan()
    eng.close()
    return plan


def test_the_plan_does_not_depend_on_the_option(pkg):
    default, moved, kept = _plan(pkg, None), _plan(pkg, 1), _plan(pkg, 0)
    assert np.array_equal(default, moved) and np.array_equal(moved, kept)
    # ... and it still describes the corner product in the tile that covers it: every J tile but the first of a subcontig has a distance-1 tile with bit (0, 7)
    jv, vv, mlo = moved[:, 0].astype(np.int64), moved[:, 1].astype(np.int64), moved[:, 3]
    dist1 = (jv - vv) == TILE_ROWS
    assert dist1.sum() == sum((s + TILE_ROWS - 1) // TILE_ROWS - 1 for s in SUBCONTIGS) == 8
    assert ((mlo[dist1] >> 7) & 1).all()
    assert sorted(jv[dist1].tolist()) == sorted(tile_boundaries())
    assert (jv == vv).sum() == 11


def test_the_exported_diagonal_map_is_unchanged(pkg):
    words = pkg.LdPruneEngine.debug_wide_diag_map()
    assert words[:, :3].tolist() == [[0, 0, 7], [2, 1, 7], [4, 3, 7], [6, 5, 7], [6, 3, 3], [2, 0, 1], [4, 0, 7], [6, 0, 7]]
    # wave 0's third column (V block 2 against J blocks 0, 1) owns nothing: the slot the corner product takes
    owned0 = int(words[0, 3]) | (int(words[0, 4]) << 32)
    assert owned0 == (1 << 0) | (1 << 8) | (1 << 9)


# ---------------------------------------------------------------- GPU: decisions on the production kernel
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
    rng = np.random.default_rng(1000 * n + 11 + KINDS.index(kind))
    raw = _fresh(rng, M, n)
    if kind == "boundary pairs":
        for b in tile_boundaries(every_second=True):      # row b copies row b - 1: the only pairs in LD lie in corner products
            _chain(rng, raw, b - 1, 2, 0.05)
    elif kind == "boundary chains":
        for b in tile_boundaries():                       # rows b - 2 .. b + 2
            _chain(rng, raw, b - 2, 5, 0.06)
    elif kind == "long":
        _chain(rng, raw, LONG_BOUNDARY - 40, 80, 0.005)   # rows b - 40 .. b + 39: r^2 still above 0.2 end to end
    assert not (raw == 3).any()
    return raw


class Rows:
    """one genotype set at one sample count, and everything the engines over it are compared with -- computed once"""

    def __init__(self, pkg, kind, n):
        self.kind, self.n = kind, n
        self.raw = genotypes(kind, n)
        self.packed = T.pack_2bit(self.raw)
        self.chr_idx = np.repeat(np.arange(len(SUBCONTIGS), dtype=np.uint32), SUBCONTIGS)
        eng = pkg.LdPruneEngine(n, WINDOW, 1, False, 0.2, order=2, device=0)
        eng.set_option("wide_min_reach", 12)
        eng.set_variants(self.chr_idx, None)
        self.lo, self.cand = eng.band()
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


RUNS = (("corner moved", {"wide_diag_corner": 1}), ("corner kept", {"wide_diag_corner": 0}), ("2 x 4 body", {"wide_diag_kernel": 0}))


def run(pkg, rows, r2, order, options):
    eng = pkg.LdPruneEngine(rows.n, WINDOW, 1, False, r2, order=order, device=0)
    eng.set_option("wide_min_reach", 12)
    for name, value in options.items():
        eng.set_option(name, value)
    eng.set_variants(rows.chr_idx, None)
    eng.load_genotypes_host(0, rows.packed, pkg.LDP_GENO_REF)
    removed = eng.run()
    pred, outside = eng.last_pred(with_outside=True)
    c = eng.counters()
    eng.close()
    return removed, pred, outside, c


def what_the_set_exercises(rows, want, r2):
    """from the reference alone, so that no set hides a failure"""
    first, second = rows.first, rows.second
    s0 = np.asarray(STARTS, dtype=np.int64)[rows.chr_idx[second]]
    tile_i, tile_j = (first - s0) // TILE_ROWS, (second - s0) // TILE_ROWS
    block_dist = (second - s0) // BLOCK - (first - s0) // BLOCK
    if rows.kind == "none":
        assert not want.any()
    elif rows.kind == "boundary pairs":
        chosen = tile_boundaries(every_second=True)
        assert int(want.sum()) == len(chosen) == 4
        assert sorted(second[want].tolist()) == chosen and (first[want] == second[want] - 1).all()     # every true pair is (b - 1, b)
        assert (tile_j[want] == tile_i[want] + 1).all() and (block_dist[want] == 1).all()               # ... in a corner product
        assert len(tile_boundaries()) == 8                                                               # corners with and without a survivor alternate
    elif rows.kind == "boundary chains":
        for b in tile_boundaries():
            near = want & (second >= b - 2) & (second <= b + 2)
            assert (near & (second < b)).any(), b                     # before the boundary: the previous diagonal tile
            assert (near & (first >= b)).any(), b                     # behind it: this diagonal tile
            assert (near & (first < b) & (second >= b)).any(), b      # across: the corner product
        assert STARTS[2] + 2 * TILE_ROWS in tile_boundaries()         # the 12-row last tile has a corner with a survivor
    else:
        crossers = want & (first < LONG_BOUNDARY) & (second >= LONG_BOUNDARY)
        assert (crossers & (block_dist == 1) & (first >= LONG_BOUNDARY - BLOCK) & (second < LONG_BOUNDARY + BLOCK)).any()   # the corner
        assert (crossers & (block_dist >= 2)).any()                   # the distance-1 tile's other products: they live on without the corner


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n,r2,order",
                         [(kind, n, r2, 2) for kind in KINDS for n in SAMPLES for r2 in (0.2, 0.5)] + [("boundary chains", n, r2, 1) for n in SAMPLES for r2 in (0.2, 0.5)])
def test_every_decision_with_the_corner_moved_and_kept(gpu_pkg, kind, n, r2, order):
    """kind "none": no LD, every corner dies at the first checkpoint.  "boundary pairs": row b copies row b - 1 at every second tile boundary -- the only pairs in
    LD lie in corner products, and corners with and without a survivor alternate.  "boundary chains": five rows across every tile boundary: pairs in LD in the
    corner, in the diagonal tile before it and in the one behind it, the 12-row last tile's among them.  "long": one 80-row chain across a tile boundary: pairs
    in LD in the corner AND in the distance-1 tile's products two blocks off the diagonal, which must live on in that tile once its corner is gone."""
    pkg = gpu_pkg
    rows = rows_of(pkg, kind, n)
    want = rows.decisions(r2)
    what_the_set_exercises(rows, want, r2)
    results = {}
    for label, options in RUNS:
        removed, pred, outside, c = run(pkg, rows, r2, order, options)
        print("pairs compared: %d (%s, n %d, r2 %g, order %d, %s; %d true; wide tiles %d, block products %d, product stages %d, skipped %d, extra %d)"
              % (len(pred), kind, n, r2, order, label, int(pred.sum()), c["wide_tiles"], c["mfma_block_products"], c["mfma_product_stages"],
                 c["mfma_skipped_product_stages"], c["mfma_extra_product_stages"]))
        assert c["candidate_pairs"] == rows.cand == len(pred)
        nd, msg = T.compare_decisions(pred, want, rows.lo, rows.stats, r2, counters=c)
        assert nd == 0, "%s\n%s" % (label, msg)
        assert int(pred.sum()) == c["pred_true"], (label, int(pred.sum()), c["pred_true"])     # no pair decided twice
        assert outside == 0
        assert np.array_equal(removed, rows.removed(r2, order)), (label, int(removed.sum()), int(rows.removed(r2, order).sum()))
        assert c["route_complete_launches"] > 0 and c["route_sparse_launches"] == 0 and c["route_general_launches"] == 0
        assert c["wide_tiles"] > 0
        results[label] = c
    for key in ("candidate_pairs", "mfma_block_products", "mfma_product_stages"):       # the plan is the same
        assert len({results[label][key] for label, _ in RUNS}) == 1, (key, [results[label][key] for label, _ in RUNS])
    if kind == "boundary pairs":
        # the distance-1 wave retires: its seven other planned products now stop at a checkpoint
        assert results["corner moved"]["mfma_skipped_product_stages"] > results["corner kept"]["mfma_skipped_product_stages"]
