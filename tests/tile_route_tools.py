"""Shared by the per-tile routing tests (test_tile_route*.py, fuzz_tile_route.py): rows whose missingness differs along the genome, and a
numpy restatement of the class rule -- the reference for LdPruneEngine.tile_classes().  Nothing here is derived from the
code under test: the restatement reads the plan (debug_wide_plan, host-only) and the rows' missing counts."""
import numpy as np

import ldtools as T

COMPLETE, SPARSE, GENERAL = 0, 1, 2
TAKEN, GIVEN = 4, 8
TILE = 256          # rows per tile side: 8 row-blocks of 32
SPARSE_FRAC = 0.005   # the engines' default "sparse_frac"


def stretch_rows(m, n, seed, stretches, second=0):
    """m complete rows of n samples with planted LD on one chromosome (+ `second` rows on another); stretches = [(first, end, rate)]: the rows
    [first, end) miss `rate` of their calls (at least one call each stretch).  Returns raw codes and the chromosome index."""
    raw = T.synth_raw_codes(m + second, n, seed=seed, missing_rate=0.0, ld_copy_prob=0.6, redraw=0.1)
    rng = np.random.default_rng(seed + 77)
    for a, b, rate in stretches:
        if b <= a:
            continue
        part = raw[a:b]
        hit = rng.random(part.shape) < rate
        if not hit.any():
            hit[rng.integers(b - a), rng.integers(n)] = True
        part[hit] = 3
        raw[a:b] = part
    chr_idx = np.concatenate([np.zeros(m, dtype=np.uint32), np.ones(second, dtype=np.uint32)])
    return raw, chr_idx


def missing_per_row(raw):
    return (raw == 3).sum(axis=1).astype(np.int64)


def _rule(miss, n, frac, allow_sparse):
    """route_kernel's rule over rows with `miss` missing calls each"""
    rows = len(miss)
    total = int(miss.sum())
    if total == 0:
        return COMPLETE
    miss_high = int(min(2.0 * frac * float(n), 4294967295.0))
    high = int((miss > miss_high).sum())
    ok = allow_sparse and (frac > 0.0) and (total <= int(frac * float(n) * float(max(rows, 1)))) and (high <= int(0.02 * float(max(rows, 1))))
    return SPARSE if ok else GENERAL


def group_word(miss, n, frac=SPARSE_FRAC, allow_sparse=True):
    """the word of a launch group that reads all the rows of `miss`"""
    return _rule(miss, n, frac, allow_sparse)


def live_rows(tile, m_rows):
    """the rows a tile multiplies: every J block whose mask row, every V block whose mask column is non-zero; clipped at jend and the row count"""
    jv, vv, jend = int(np.int32(tile[0])), int(np.int32(tile[1])), int(tile[2])
    mask = int(tile[3]) | (int(tile[4]) << 32)
    rows = set()
    for a in range(8):
        if (mask >> (8 * a)) & 0xff:
            rows.update(range(jv + 32 * a, jv + 32 * a + 32))
    for b in range(8):
        if any((mask >> (8 * a + b)) & 1 for a in range(8)):
            rows.update(range(vv + 32 * b, vv + 32 * b + 32))
    end = min(jend, m_rows)
    return np.array(sorted(r for r in rows if 0 <= r < end), dtype=np.int64)


def expected_classes(plan, miss, n, word, frac=SPARSE_FRAC, allow_sparse=True, corner=True):
    """one byte per tile of `plan` (debug_wide_plan()): bits 0-1 min(word, class of the tile's own rows), bit 2 / bit 3 the corner product taken / given
    -- handed over exactly where the distance-1 tile and the diagonal tile of one J tile are both complete"""
    m_rows = len(miss)
    own = np.array([_rule(miss[live_rows(t, m_rows)], n, frac, allow_sparse) for t in plan], dtype=np.uint8)
    cls = np.minimum(own, np.uint8(word)).astype(np.uint8)
    out = cls.copy()
    if corner:
        diag_of = {int(t[0]): i for i, t in enumerate(plan) if t[0] == t[1]}
        for i, t in enumerate(plan):
            if (int(np.int32(t[0])) - int(np.int32(t[1])) == TILE) and ((int(t[3]) >> 7) & 1) and (int(t[0]) in diag_of):
                d = diag_of[int(t[0])]
                if own[i] == COMPLETE:
                    # (the 32 rows in front of the diagonal tile and all of its own rows are rows of the distance-1 tile)
                    assert own[d] == COMPLETE, "a complete distance-1 tile next to an incomplete diagonal tile: the plan is not what the rule assumes"
                    out[i] |= GIVEN
                    out[d] |= TAKEN
    return out


def class_counts(classes):
    c = classes & 3
    return {"tiles_complete": int((c == COMPLETE).sum()), "tiles_sparse": int((c == SPARSE).sum()), "tiles_general": int((c == GENERAL).sum()),
            "corner_products": int(((classes & TAKEN) != 0).sum())}


def random_layout(seed, n=700):
    """one chromosome of an odd number of rows cut into five stretches -- complete, 0.1 % or 5 % missing -- whose edges are drawn on multiples of 256
    (tile edges), on multiples of 32 (row-block edges) and anywhere; returns raw codes, the chromosome index and the stretches"""
    rng = np.random.default_rng(1000 + seed)
    m = 1601 + 2 * int(rng.integers(0, 200))
    cuts = set()
    while len(cuts) < 4:
        kind = int(rng.integers(0, 3))
        unit = (256, 32, 1)[kind]
        c = unit * int(rng.integers(1, (m - 1) // unit + 1))
        if 0 < c < m:
            cuts.add(c)
    edges = [0] + sorted(cuts) + [m]
    rates = [0.0, 0.001, 0.05, 0.0, (0.0, 0.001, 0.05)[int(rng.integers(0, 3))]]
    rng.shuffle(rates)
    stretches = [(edges[k], edges[k + 1], rates[k]) for k in range(5) if rates[k] > 0.0]
    raw, chr_idx = stretch_rows(m, n, seed=7000 + seed, stretches=stretches)
    return raw, chr_idx, stretches


RANDOM_SEEDS = list(range(1, 21))
WINDOW = 600


class CapturingPkg:
    """the package with an engine class that keeps tile_routes() / tile_classes() / debug_wide_plan() of its last run when it is closed --
    so that test_pair_decisions.decide(), which closes its engine, can be reused as it is"""

    def __init__(self, pkg):
        self._pkg = pkg
        self.captured = []
        outer = self

        class Engine(pkg.LdPruneEngine):
            def close(self):
                if self._h:
                    rec = {"routes": self.tile_routes(), "plan": self.debug_wide_plan()}
                    try:
                        rec["classes"] = self.tile_classes()
                    except pkg.LdpError as err:
                        rec["classes"] = None
                        rec["classes_error"] = err.code
                    outer.captured.append(rec)
                super().close()

        self.LdPruneEngine = Engine

    def __getattr__(self, name):
        return getattr(self._pkg, name)
